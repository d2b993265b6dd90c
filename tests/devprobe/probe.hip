// probe.hip -- device probes of the cross-lane building blocks of csrc/wave.hpp and csrc/stage.hpp.
//
// Test infrastructure (tests/test_gpu_lane_blocks.py), never loaded by the product path.  The host simulation
// instantiates the kernel templates with one lane, so everything that exists only for more than one lane -- the DPP /
// readlane reduction trees, lane_xor_fetch, RowSum on narrow groups, the ballot/prefix partition, the register sorting
// network, the ballot counts and the register-blocked rank scan -- is run here, one block and one policy at a time,
// on inputs the test chooses and against expectations the test computes (tests/lane_reference.py).
//
// C ABI: one extern "C" function per probe.  Each takes HOST pointers, checks sizes on the host (negative return code,
// nothing launched), allocates, copies in, launches one small grid, synchronises, copies out, frees, and returns the
// hipError_t.  Every output buffer is kPad bytes longer than its payload; payload and pad are filled with the byte kFill
// before the launch and copied back whole, so the caller can tell "never written" and "written past the end" from a
// value.  No kernel here can wait for another workgroup: bounded loops, no atomics, barriers in uniform control flow only.
#include "stage.hpp"

#include "call.hpp"

using namespace lcfe;

namespace {

// what a policy offers, and the workgroup it is launched as
template <class W>
struct traits { static constexpr int T = 64; static constexpr bool ballot = true, bcast = true, first = false; };
template <>
struct traits<WaveOfBlock> { static constexpr int T = 256; static constexpr bool ballot = true, bcast = false, first = true; };
template <int GS>
struct traits<GroupDev<GS>> { static constexpr int T = 64; static constexpr bool ballot = true, bcast = false, first = false; };
template <int TT>
struct traits<BlockDev<TT>> { static constexpr int T = TT; static constexpr bool ballot = false, bcast = false, first = true; };
template <class W>
struct has_prefix { static constexpr bool value = traits<W>::ballot; };
template <>
struct has_prefix<WaveOfBlock> { static constexpr bool value = false; };

// policy ids of the ABI
#define PROBE_ALL_POLICIES(X) \
    X(0, WaveDev) X(1, LongDev) X(2, WaveOfBlock) X(3, GroupDev<8>) X(4, GroupDev<4>) X(5, GroupDev<2>) \
    X(6, BlockDev<256>) X(7, BlockDev<512>) X(8, BlockDev<1024>)

// ---- sum / max / min, double and int, as seen by every thread.  od, oi: [block][sum, max, min][T]
template <class W>
__global__ void __launch_bounds__(traits<W>::T) k_reduce(const double* ds, const double* dm, const int* is, const int* im, double* od, int* oi) {
    constexpr int T = traits<W>::T;
    const int tid = threadIdx.x;
    const size_t at = (size_t)blockIdx.x * T + tid;
    double* o = od + (size_t)blockIdx.x * 3 * T;
    int* p = oi + (size_t)blockIdx.x * 3 * T;
    o[tid] = W::sum(ds[at]);
    o[T + tid] = W::max(dm[at]);
    o[2 * T + tid] = W::min(dm[at]);
    p[tid] = W::sum(is[at]);
    p[T + tid] = W::max(im[at]);
    p[2 * T + tid] = W::min(im[at]);
}
template <class W>
int run_reduce(int nb, const double* ds, const double* dm, const int* is, const int* im, double* od, int* oi) {
    constexpr int T = traits<W>::T;
    Call c;
    const size_t n = (size_t)nb * T;
    const double *a = c.in(ds, n), *b = c.in(dm, n);
    const int *d = c.in(is, n), *e = c.in(im, n);
    double* o = c.out(od, 3 * n);
    int* p = c.out(oi, 3 * n);
    if (c.ok()) k_reduce<W><<<nb, T>>>(a, b, d, e, o, p);
    return c.finish();
}

// ---- any / all / ballot / prefix / bcast / bcast_from_first_wave.
// oi: [block][any, all, prefix, bcast(int)][T]; ob: [block][T]; od: [block][bcast(double), from_first_wave][T].  What a
// policy does not offer stays sentinel.
template <class W>
__global__ void __launch_bounds__(traits<W>::T) k_vote(const unsigned char* pred, const double* v, const int* src, int* oi, unsigned long long* ob, double* od) {
    constexpr int T = traits<W>::T;
    const int tid = threadIdx.x;
    const size_t blk = blockIdx.x, at = blk * T + tid;
    const bool p = pred[at] != 0;
    int* qi = oi + blk * 4 * T;
    double* qd = od + blk * 2 * T;
    qi[tid] = W::any(p) ? 1 : 0;
    qi[T + tid] = W::all(p) ? 1 : 0;
    if constexpr (traits<W>::ballot) {
        const unsigned long long m = W::ballot(p);
        ob[at] = m;
        if constexpr (has_prefix<W>::value) qi[2 * T + tid] = W::prefix(m);
    }
    if constexpr (traits<W>::bcast) {
        const int s = src[blk];
        const double x = v[at];
        qd[tid] = W::bcast(x, s);
        qi[3 * T + tid] = W::bcast((int)__builtin_bit_cast(long long, x), s);
    }
    // the argument is uniform over each wavefront and differs between them
    if constexpr (traits<W>::first) qd[T + tid] = W::bcast_from_first_wave(v[blk * T + (tid & ~63)]);
}
template <class W>
int run_vote(int nb, const unsigned char* pred, const double* v, const int* src, int* oi, unsigned long long* ob, double* od) {
    constexpr int T = traits<W>::T;
    for (int k = 0; k < nb; ++k)
        if (src[k] < 0 || src[k] > 63) return kBadSize;
    Call c;
    const size_t n = (size_t)nb * T;
    const unsigned char* a = c.in(pred, n);
    const double* b = c.in(v, n);
    const int* s = c.in(src, nb);
    int* qi = c.out(oi, 4 * n);
    unsigned long long* qb = c.out(ob, n);
    double* qd = c.out(od, 2 * n);
    if (c.ok()) k_vote<W><<<nb, T>>>(a, b, s, qi, qb, qd);
    return c.finish();
}

// ---- xfetch<MASK> for every MASK in 1..LANES-1.  out: [MASK - 1][64]
template <class W, int MASK>
__device__ __forceinline__ void xfetch_from(double v, double* out) {
    if constexpr (MASK < W::LANES) {
        out[(MASK - 1) * 64 + threadIdx.x] = W::template xfetch<MASK>(v);
        xfetch_from<W, MASK + 1>(v, out);
    }
}
template <class W>
__global__ void __launch_bounds__(64) k_xfetch(const double* x, double* out) { xfetch_from<W, 1>(x[threadIdx.x], out); }
template <class W>
int run_xfetch(const double* x, double* out) {
    Call c;
    const double* a = c.in(x, 64);
    double* o = c.out(out, (size_t)(W::LANES - 1) * 64);
    if (c.ok()) k_xfetch<W><<<1, 64>>>(a, o);
    return c.finish();
}

// ---- group collectives while the groups of one wave diverge: group g runs (g % 5) + 1 trips over x[trip][64],
// pred[trip][64] and stores the last trip's results.  od: [sum, max][64]; ob: [64]; oi: [any][64]
template <int GS>
__global__ void __launch_bounds__(64) k_diverge(const double* x, const unsigned char* pred, double* od, unsigned long long* ob, int* oi) {
    using W = GroupDev<GS>;
    const int tid = threadIdx.x;
    const int trips = W::group_id() % 5 + 1;
    double s = 0.0, mx = 0.0;
    unsigned long long bl = 0;
    int an = 0;
    for (int k = 0; k < trips; ++k) {
        const double v = x[k * 64 + tid];
        const bool p = pred[k * 64 + tid] != 0;
        s = W::sum(v);
        mx = W::max(v);
        bl = W::ballot(p);
        an = W::any(p) ? 1 : 0;
        W::sync();
    }
    od[tid] = s;
    od[64 + tid] = mx;
    ob[tid] = bl;
    oi[tid] = an;
}
template <int GS>
int run_diverge(const double* x, const unsigned char* pred, double* od, unsigned long long* ob, int* oi) {
    Call c;
    const double* a = c.in(x, 5 * 64);
    const unsigned char* b = c.in(pred, 5 * 64);
    double* qd = c.out(od, 2 * 64);
    unsigned long long* qb = c.out(ob, 64);
    int* qi = c.out(oi, 64);
    if (c.ok()) k_diverge<GS><<<1, 64>>>(a, b, qd, qb, qi);
    return c.finish();
}

// ---- RowSum: row r = x[r][0..m[r]) is summed by one group with the loop form documented above row_slots in
// wave.hpp.  out: [row][GS], the total as seen by every lane of the group
template <int GS>
__global__ void __launch_bounds__(64) k_rowsum(const double* x, const int* ms, int nrows, int cap, double* out) {
    using W = GroupDev<GS>;
    constexpr int NS = row_slots<W>::value;
    const int row = blockIdx.x * W::NGROUPS + W::group_id();
    if (row >= nrows) return;
    const double* xr = x + (size_t)row * cap;
    const int m = ms[row];
    RowSum<W> acc;
    for (int i0 = W::lane(); i0 < m; i0 += NS * W::LANES)
        for (int sl = 0; sl < NS; ++sl) {
            const int i = i0 + sl * W::LANES;
            if (i >= m) break;
            acc[sl] += xr[i];
        }
    out[(size_t)row * GS + W::lane()] = acc.total();
}
template <int GS>
int run_rowsum(int nrows, int cap, const double* x, const int* ms, double* out) {
    constexpr int NG = 64 / GS;
    const int nb = (nrows + NG - 1) / NG;
    if (nrows < 1 || cap < 1 || nb > kMaxBlocks) return kBadSize;
    for (int r = 0; r < nrows; ++r)
        if (ms[r] < 0 || ms[r] > cap) return kBadSize;
    Call c;
    const double* a = c.in(x, (size_t)nrows * cap);
    const int* b = c.in(ms, nrows);
    double* o = c.out(out, (size_t)nrows * GS);
    if (c.ok()) k_rowsum<GS><<<nb, 64>>>(a, b, nrows, cap, o);
    return c.finish();
}

// ---- stage_object.  WaveDev: the ObjLds<128> lives in LDS, is filled with the sentinel first and copied out whole.
// LongDev: an ObjLds<2048> in global memory (sentinel-filled by the host side of the probe).
constexpr int kStageCapWave = 128, kStageCapLong = 2048;
__global__ void __launch_bounds__(64) k_stage_wave(ObjIn in, unsigned char* out) {
    __shared__ ObjLds<kStageCapWave> L;
    unsigned char* raw = reinterpret_cast<unsigned char*>(&L);
    for (unsigned i = threadIdx.x; i < sizeof(L); i += 64) raw[i] = (unsigned char)kFill;
    __syncthreads();
    stage_object<WaveDev, kStageCapWave>(in, L);
    __syncthreads();
    for (unsigned i = threadIdx.x; i < sizeof(L); i += 64) out[i] = raw[i];
}
__global__ void __launch_bounds__(64) k_stage_long(ObjIn in, ObjLds<kStageCapLong>* L) { stage_object<LongDev, kStageCapLong>(in, *L); }

template <int CAP>
void stage_layout(long long* o) {
    using L = ObjLds<CAP>;
    const long long v[13] = {CAP, (long long)sizeof(L), offsetof(L, t), offsetof(L, f), offsetof(L, e), offsetof(L, bt), offsetof(L, bf),
                             offsetof(L, be), offsetof(L, bidx), offsetof(L, b), offsetof(L, boff), offsetof(L, n), offsetof(L, sorted)};
    for (int k = 0; k < 13; ++k) o[k] = v[k];
}

// ---- group_sort_values: unit u (one group) sorts x[u][0..m[u]) into out[u]; a row holds LANES * KPL values
template <class W, int KPL>
__global__ void __launch_bounds__(64) k_sort(const double* x, const int* ms, double* out) {
    constexpr int ROW = W::LANES * KPL;
    const size_t u = (size_t)blockIdx.x * W::NGROUPS + W::group_id();
    group_sort_values<W, KPL>(x + u * ROW, ms[u], out + u * ROW);
}
template <class W, int KPL>
int run_sort(int nb, const double* x, const int* ms, double* out) {
    constexpr int ROW = W::LANES * KPL;
    const size_t nu = (size_t)nb * W::NGROUPS;
    for (size_t u = 0; u < nu; ++u)
        if (ms[u] < 0 || ms[u] > ROW) return kBadSize;
    Call c;
    const double* a = c.in(x, nu * ROW);
    const int* b = c.in(ms, nu);
    double* o = c.out(out, nu * ROW);
    if (c.ok()) k_sort<W, KPL><<<nb, 64>>>(a, b, o);
    return c.finish();
}

// ---- wave_select_ranks: unit u selects ranks[u][0..NT) of x[u][0..m[u]); rows of x and rk hold 8 * LANES + 8 values;
// the key scratch is LDS, as in the kernels
template <class W, int NT, bool RK>
__global__ void __launch_bounds__(64) k_select(const double* x, const int* ms, const int* ranks, double* sel, int* rk) {
    constexpr int ROW = 8 * W::LANES + 8;
    __shared__ unsigned long long keys[W::NGROUPS * ROW];
    const size_t u = (size_t)blockIdx.x * W::NGROUPS + W::group_id();
    wave_select_ranks<W, NT, RK>(x + u * ROW, ms[u], keys + W::group_id() * ROW, ranks + u * NT, sel + u * NT, RK ? rk + u * ROW : nullptr);
}
template <class W, int NT, bool RK>
int run_select(int nb, const double* x, const int* ms, const int* ranks, double* sel, int* rk) {
    constexpr int ROW = 8 * W::LANES + 8;
    const size_t nu = (size_t)nb * W::NGROUPS;
    for (size_t u = 0; u < nu; ++u)
        if (ms[u] < 0 || ms[u] > ROW) return kBadSize;
    Call c;
    const double* a = c.in(x, nu * ROW);
    const int* b = c.in(ms, nu);
    const int* r = c.in(ranks, nu * NT);
    double* s = c.out(sel, nu * NT);
    int* k = c.out(rk, nu * ROW);
    if (c.ok()) k_select<W, NT, RK><<<nb, 64>>>(a, b, r, s, k);
    return c.finish();
}

// ---- mad_of_sorted and wave_argmax_first: rows of 4 * LANES values, the result as seen by every lane.  out: [unit][LANES]
template <class W>
__global__ void __launch_bounds__(64) k_mad(const double* s, const int* ms, const double* med, double* out) {
    constexpr int ROW = 4 * W::LANES;
    const size_t u = (size_t)blockIdx.x * W::NGROUPS + W::group_id();
    out[u * W::LANES + W::lane()] = mad_of_sorted<W>(s + u * ROW, ms[u], med[u]);
}
template <class W>
__global__ void __launch_bounds__(64) k_argmax(const double* x, const int* ms, int* out) {
    constexpr int ROW = 4 * W::LANES;
    const size_t u = (size_t)blockIdx.x * W::NGROUPS + W::group_id();
    out[u * W::LANES + W::lane()] = wave_argmax_first<W>(x + u * ROW, ms[u]);
}
template <class W>
int run_mad(int nb, const double* s, const int* ms, const double* med, double* out) {
    constexpr int ROW = 4 * W::LANES;
    const size_t nu = (size_t)nb * W::NGROUPS;
    for (size_t u = 0; u < nu; ++u)
        if (ms[u] < 1 || ms[u] > ROW) return kBadSize;       // mad_of_sorted reads s[0] and s[h]: m >= 1
    Call c;
    const double* a = c.in(s, nu * ROW);
    const int* b = c.in(ms, nu);
    const double* d = c.in(med, nu);
    double* o = c.out(out, nu * W::LANES);
    if (c.ok()) k_mad<W><<<nb, 64>>>(a, b, d, o);
    return c.finish();
}
template <class W>
int run_argmax(int nb, const double* x, const int* ms, int* out) {
    constexpr int ROW = 4 * W::LANES;
    const size_t nu = (size_t)nb * W::NGROUPS;
    for (size_t u = 0; u < nu; ++u)
        if (ms[u] < 0 || ms[u] > ROW) return kBadSize;
    Call c;
    const double* a = c.in(x, nu * ROW);
    const int* b = c.in(ms, nu);
    int* o = c.out(out, nu * W::LANES);
    if (c.ok()) k_argmax<W><<<nb, 64>>>(a, b, o);
    return c.finish();
}

bool blocks_ok(int nb) { return nb >= 1 && nb <= kMaxBlocks; }

}  // namespace

extern "C" {

int devprobe_pad() { return kPad; }
int devprobe_fill() { return kFill; }
int devprobe_device_count() {
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

// threads of the workgroup `policy` is launched as (0 for an unknown id)
int devprobe_threads(int policy) {
    switch (policy) {
#define X(id, W) case id: return traits<W>::T;
        PROBE_ALL_POLICIES(X)
#undef X
    }
    return 0;
}

int devprobe_reduce(int policy, int nblocks, const double* dsum, const double* dmm, const int* isum, const int* imm, double* od, int* oi) {
    if (!blocks_ok(nblocks)) return kBadSize;
    switch (policy) {
#define X(id, W) case id: return run_reduce<W>(nblocks, dsum, dmm, isum, imm, od, oi);
        PROBE_ALL_POLICIES(X)
#undef X
    }
    return kBadShape;
}

int devprobe_vote(int policy, int nblocks, const unsigned char* pred, const double* v, const int* src, int* oi, unsigned long long* ob, double* od) {
    if (!blocks_ok(nblocks)) return kBadSize;
    switch (policy) {
#define X(id, W) case id: return run_vote<W>(nblocks, pred, v, src, oi, ob, od);
        PROBE_ALL_POLICIES(X)
#undef X
    }
    return kBadShape;
}

int devprobe_xfetch(int policy, const double* x, double* out) {
    switch (policy) {
        case 0: return run_xfetch<WaveDev>(x, out);
        case 3: return run_xfetch<GroupDev<8>>(x, out);
        case 4: return run_xfetch<GroupDev<4>>(x, out);
        case 5: return run_xfetch<GroupDev<2>>(x, out);
    }
    return kBadShape;
}

int devprobe_diverge(int gs, const double* x, const unsigned char* pred, double* od, unsigned long long* ob, int* oi) {
    switch (gs) {
        case 8: return run_diverge<8>(x, pred, od, ob, oi);
        case 4: return run_diverge<4>(x, pred, od, ob, oi);
        case 2: return run_diverge<2>(x, pred, od, ob, oi);
    }
    return kBadShape;
}

int devprobe_rowsum(int gs, int nrows, int cap, const double* x, const int* ms, double* out) {
    switch (gs) {
        case 8: return run_rowsum<8>(nrows, cap, x, ms, out);
        case 4: return run_rowsum<4>(nrows, cap, x, ms, out);
        case 2: return run_rowsum<2>(nrows, cap, x, ms, out);
    }
    return kBadShape;
}

// o[13]: CAP, sizeof, then the offsets of t f e bt bf be bidx b boff n sorted.  policy 0 = WaveDev / ObjLds<128> in LDS,
// 1 = LongDev / ObjLds<2048> in global memory
int devprobe_stage_layout(int policy, long long* o) {
    if (policy == 0) stage_layout<kStageCapWave>(o);
    else if (policy == 1) stage_layout<kStageCapLong>(o);
    else return kBadShape;
    return 0;
}

// out: sizeof(ObjLds) + pad bytes
int devprobe_stage(int policy, int n, const double* t, const double* f, const double* e, const unsigned char* b, unsigned char* out) {
    if (policy != 0 && policy != 1) return kBadShape;
    const int cap = policy == 0 ? kStageCapWave : kStageCapLong;
    if (n < 0 || n > cap) return kBadSize;
    Call c;
    ObjIn in;
    in.t = c.in(t, n);
    in.f = c.in(f, n);
    in.e = c.in(e, n);
    in.b = c.in(b, n);
    in.n = n;
    in.z = 0.0;
    unsigned char* o = c.out(out, policy == 0 ? sizeof(ObjLds<kStageCapWave>) : sizeof(ObjLds<kStageCapLong>));
    if (c.ok()) {
        if (policy == 0) k_stage_wave<<<1, 64>>>(in, o);
        else k_stage_long<<<1, 64>>>(in, reinterpret_cast<ObjLds<kStageCapLong>*>(o));
    }
    return c.finish();
}

// shape: 0 (GroupDev<8>, 4)  1 (GroupDev<8>, 8)  2 (WaveDev, 2)  3 (WaveDev, 4)  4 (WaveDev, 8)
int devprobe_sort(int shape, int nblocks, const double* x, const int* ms, double* out) {
    if (!blocks_ok(nblocks)) return kBadSize;
    switch (shape) {
        case 0: return run_sort<GroupDev<8>, 4>(nblocks, x, ms, out);
        case 1: return run_sort<GroupDev<8>, 8>(nblocks, x, ms, out);
        case 2: return run_sort<WaveDev, 2>(nblocks, x, ms, out);
        case 3: return run_sort<WaveDev, 4>(nblocks, x, ms, out);
        case 4: return run_sort<WaveDev, 8>(nblocks, x, ms, out);
    }
    return kBadShape;
}

// policy 0 = WaveDev, 3 = GroupDev<8>; nt = 2, 6, or 26 (= CESIUM_NSEL of csrc/cesium.hpp, instantiated with RK)
int devprobe_select(int policy, int nt, int nblocks, const double* x, const int* ms, const int* ranks, double* sel, int* rk) {
    if (!blocks_ok(nblocks)) return kBadSize;
    if (policy == 0) {
        if (nt == 2) return run_select<WaveDev, 2, false>(nblocks, x, ms, ranks, sel, rk);
        if (nt == 6) return run_select<WaveDev, 6, false>(nblocks, x, ms, ranks, sel, rk);
        if (nt == 26) return run_select<WaveDev, 26, true>(nblocks, x, ms, ranks, sel, rk);
    } else if (policy == 3) {
        if (nt == 2) return run_select<GroupDev<8>, 2, false>(nblocks, x, ms, ranks, sel, rk);
        if (nt == 6) return run_select<GroupDev<8>, 6, false>(nblocks, x, ms, ranks, sel, rk);
        if (nt == 26) return run_select<GroupDev<8>, 26, true>(nblocks, x, ms, ranks, sel, rk);
    }
    return kBadShape;
}

int devprobe_mad(int policy, int nblocks, const double* s, const int* ms, const double* med, double* out) {
    if (!blocks_ok(nblocks)) return kBadSize;
    if (policy == 0) return run_mad<WaveDev>(nblocks, s, ms, med, out);
    if (policy == 3) return run_mad<GroupDev<8>>(nblocks, s, ms, med, out);
    return kBadShape;
}

int devprobe_argmax(int policy, int nblocks, const double* x, const int* ms, int* out) {
    if (!blocks_ok(nblocks)) return kBadSize;
    if (policy == 0) return run_argmax<WaveDev>(nblocks, x, ms, out);
    if (policy == 3) return run_argmax<GroupDev<8>>(nblocks, x, ms, out);
    return kBadShape;
}

}  // extern "C"
