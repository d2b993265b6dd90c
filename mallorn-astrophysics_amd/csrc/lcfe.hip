// lcfe.hip -- gfx950 kernels + C-ABI of liblcfe.so (see include/lcfe.h).
//
// Execution model: one light curve per 64-lane wavefront, one wavefront per workgroup, a
// persistent grid that strides over the objects.  Per feature set the object's working set
// (staged samples, sorted views, Jacobians, Gram matrices) lives in LDS; HBM is touched once for
// the CSR slice and once for the output row.  Objects are binned into LDS tiers by point count
// (CAP = 128 .. 2048) by one small kernel per call that writes an index list per tier; each tier is
// one launch over its list, so short light curves run at high occupancy and long ones still fit.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/lcfe.h"
#include "feature_sets.hpp"
#include "workspace.hpp"
#include "tickets.hpp"
#include "stat_lean.hpp"
#include "stat_lanes.hpp"
#include "gp1d.hpp"
#include "gp1d_points.hpp"
#include "gp1d_rows.hpp"
#include "gp_tiers.hpp"
#include "gp1d_tiers.hpp"
#include "augment.hpp"
#include "gp_resample.hpp"
#include "sequence.hpp"

using namespace lcfe;

namespace {

thread_local std::string g_err;

// Restores the caller's current device on every exit path of an entry point that had to switch devices.
struct DeviceGuard {
    int prev = -1;
    bool armed = false;
    int enter(int device) {
        if (device < 0) return 0;
        if (hipGetDevice(&prev) != hipSuccess) return 1;
        if (prev == device) return 0;
        if (hipSetDevice(device) != hipSuccess) return 1;
        armed = true;
        return 0;
    }
    ~DeviceGuard() { if (armed) (void)hipSetDevice(prev); }
};

int fail(const char* what, hipError_t e, const char* file, int line) {
    char buf[512];
    snprintf(buf, sizeof buf, "%s failed: %s (%s:%d)", what, hipGetErrorString(e), file, line);
    g_err = buf;
    return 1;
}
int fail_msg(const std::string& m) {
    g_err = m;
    return 2;
}
#define HIP_TRY(expr)                                                  \
    do {                                                               \
        hipError_t e_ = (expr);                                        \
        if (e_ != hipSuccess) return fail(#expr, e_, __FILE__, __LINE__); \
    } while (0)

int g_num_cu[16] = {0};
std::mutex g_num_cu_mutex;

int num_cus(int dev) {
    if (dev < 0 || dev >= 16) return 256;
    std::lock_guard<std::mutex> lock(g_num_cu_mutex);
    if (!g_num_cu[dev]) {
        hipDeviceProp_t p;
        if (hipGetDeviceProperties(&p, dev) == hipSuccess) g_num_cu[dev] = p.multiProcessorCount;
        else g_num_cu[dev] = 256;
    }
    return g_num_cu[dev];
}

// The streams dst[0..n) wait for what has been enqueued on src so far.  The event is short-lived: one that was recorded is
// released by the runtime once the recorded work has completed, so destroying it right after the waits were enqueued is safe.
int stream_wait(const hipStream_t* dst, int n, hipStream_t src) {
    hipEvent_t e;
    HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    hipError_t err = hipEventRecord(e, src);
    for (int k = 0; k < n && err == hipSuccess; ++k) err = hipStreamWaitEvent(dst[k], e, 0);
    (void)hipEventDestroy(e);
    return (err == hipSuccess) ? 0 : fail("stream_wait", err, __FILE__, __LINE__);
}
int stream_wait(hipStream_t dst, hipStream_t src) { return stream_wait(&dst, 1, src); }

// One persistent launch: as many workgroups as the occupancy query says the chip holds (grid_for: caps, clamp to the
// tickets of work, nothing to launch for no work), handed `args`.  Caps of 0 are no caps.
struct GridCaps {
    int per_cu = 0;
    int64_t grid = 0;
};
template <class... P, class... A>
int launch_grid(void (*kernel)(P...), int threads, GridCaps caps, int64_t work_items, int per_ticket, hipStream_t stream, int dev,
                A... args) {
    int per_cu = 0;
    HIP_TRY(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0));
    if (per_cu < 1) per_cu = 1;
    if (caps.per_cu > 0 && caps.per_cu < per_cu) per_cu = caps.per_cu;
    const int64_t grid = grid_for(num_cus(dev), per_cu, caps.grid, work_items, per_ticket);
    if (grid < 1) return 0;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(threads), 0, stream, args...);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- binning: index lists per LDS tier (feature sets) and per Gram-matrix tier (GP)
// (the lists, the slots of the counts and tickets and the regions behind them: workspace.hpp; BatchView, Bins: tickets.hpp)
constexpr int kBinThreads = 1024;

// What every launcher of a set gets, built once per set by lcfe_extract_device: the batch and its bins, where the set's
// columns and status words go, its stream, and its share of the workspace; the launchers are its members.
struct FitWs;
struct PlWs;
struct SetLaunch {
    const BatchView& B;
    const Bins& bins;
    int64_t max_len;
    SetOut O;
    hipStream_t stream;
    int dev;
    int* n_launch;
    unsigned long long* tickets;
    char* long_slabs;
    // the five sets with launch sequences of their own, and every other set
    int launch_stat(hipStream_t s1, hipStream_t s2) const;
    template <class Fam> int launch_fits(const typename Fam::Ws& F) const;     // BazinFits, DeclineFits
    int launch_gp(const hipStream_t* gs, int ngs, double* const* kslab) const;
    int launch_gp1d(double* kslab) const;
    template <int SET> int launch_set() const;
    // single launches (launch_grid) with the fields above as the kernel's arguments
    template <int SET, int CAP> int tier(int bin, int nan_from, hipStream_t q, unsigned long long* tk, int64_t cap = 0) const;
    template <int SET> int long_tier(int l0, int l1, int l2) const;
    template <class K, class Ws> int fit_stream(K kernel, int tier, int fits_per_object, int ticket_base, const Ws& F) const;
    template <int CAP> int stat_lean(int bin, hipStream_t q, unsigned long long* tk, int64_t cap = 0) const;
    template <int NP, bool GLOBAL_K> int gp_tier(int ti, int nan_from, hipStream_t q, double* kscratch, int64_t cap) const;
    template <int NP, int ROWCAP, int T, int WNP, int MW> int gp1d_tier(int ti, int nan_from, double* kslab = nullptr) const;
};

__device__ __forceinline__ int set_bin_of(int64_t n) {
    return (n <= 128) ? 0 : (n <= 256) ? 1 : (n <= 512) ? 2 : (n <= 1024) ? 3 : (n <= 2048) ? 4 : 6;
}
// (the GP sets bin by gp_bin_of of gp_tier_table.hpp: a window on the ROW count of the object, >= its valid points)

// One block bins 1024 consecutive objects: ballots give the rank inside a wave, an LDS scan the
// wave's offset inside the block, one atomicAdd per (block, bin) the block's slice of the list --
// so a list keeps file order inside every 1024-object block (CSR locality for the tier kernels).
__global__ __launch_bounds__(kBinThreads) void bin_kernel(const int64_t* offsets, int64_t n_obj, int* lists, int* counts) {
    __shared__ int wcount[kBinThreads / 64][2 * kNumBins];
    __shared__ int base[2 * kNumBins];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t i = (int64_t)blockIdx.x * kBinThreads + threadIdx.x;
    int bin[2] = {-1, -1}, rank[2] = {0, 0};
    if (i < n_obj) {
        const int64_t n = offsets[i + 1] - offsets[i];
        bin[0] = set_bin_of(n);
        bin[1] = gp_bin_of(n);
    }
#pragma unroll
    for (int g = 0; g < 2; ++g)
#pragma unroll
        for (int b = 0; b < kNumBins; ++b) {
            const unsigned long long m = __ballot(bin[g] == b);
            if (bin[g] == b) rank[g] = WaveDev::prefix(m);
            if (lane == 0) wcount[wave][g * kNumBins + b] = popcll(m);
        }
    __syncthreads();
    if (threadIdx.x < 2 * kNumBins) {
        int total = 0;
        for (int w = 0; w < kBinThreads / 64; ++w) {
            const int c = wcount[w][threadIdx.x];
            wcount[w][threadIdx.x] = total;
            total += c;
        }
        base[threadIdx.x] = total ? atomicAdd(&counts[threadIdx.x], total) : 0;
    }
    __syncthreads();
#pragma unroll
    for (int g = 0; g < 2; ++g)
        if (bin[g] >= 0) {
            const int k = tier_list(g, bin[g]);
            lists[(int64_t)k * n_obj + base[k] + wcount[wave][k] + rank[g]] = (int)i;
        }
}

// NaN rows + status -100 for the objects of bins [from, kNumBins) of group `g` (too long for the
// tiers this launch sequence covers); every block of the last tier's launch takes a share.
// (the view by value: behind a reference gp_kernel<512> spilled three registers more)
template <class W>
__device__ void nan_fill_bins(const Bins& bins, int g, int from, SetOut O, int ncol, int nst) {
    for (int b = from; b < kNumBins; ++b) {
        const int c = bins.count(tier_list(g, b));
        const int* list = bins.list(tier_list(g, b));
        for (int pos = blockIdx.x; pos < c; pos += gridDim.x) O.unavailable<W>(list[pos], ncol, nst);
    }
}

// One launch = one (feature set, LDS tier): the objects of the tier's index list are handed out
// through a device-side ticket counter (zeroed once per call) -- fit costs are heavy-tailed (nfev
// 5..2000), so a static round-robin would leave most waves idle behind the unluckiest one.  One
// ticket = `chunk` consecutive list entries (a single counter saturates near 90 tickets/us, so the
// cheap streaming sets take 8 objects per ticket; the fits take one); the chunk's list entries and
// CSR offsets are fetched by its first lanes in one go.  The launch of the last tier also writes the
// NaN rows of the objects that are too long for it (bins >= nan_from).
// minimum waves per SIMD the register allocation must leave room for (SetTraits::waves128; only the 128-row tier: the
// larger tiers are limited to one wave per SIMD by their LDS footprint anyway)
template <int SET, int CAP> struct set_waves { static constexpr int N = (CAP <= 128) ? SetTraits<SET>::waves128 : 1; };

template <int SET, int CAP>
__global__ __launch_bounds__(64, (set_waves<SET, CAP>::N)) void set_kernel(BatchView B, Bins bins, int bin, int nan_from, SetOut O,
                                                 unsigned long long* ticket, int chunk) {
    __shared__ SetLds<SET, CAP> ws;
    __shared__ long long next_ticket;
    using W = WaveDev;
    const int ncol = SetTraits<SET>::ncols;
    const int nst = SetTraits<SET>::nstatus;
    const int count = bins.count(bin);
    const int* list = bins.list(bin);
    // a sparsely filled tier hands out smaller tickets, so that every wave gets several of them
    chunk = ticket_chunk(count, chunk, 4, 1);
    LCFE_PT_INIT();
    LCFE_PT0();
    for (;;) {
        const int64_t base = block_ticket(ticket, next_ticket) * chunk;
        if (base >= count) break;
        const int nk = (count - base < chunk) ? (int)(count - base) : chunk;
        TicketChunk tc;
        tc.load(list, base, nk, B);
        for (int k = 0; k < nk; ++k) {
            const auto [i, s, n] = tc.object(k);
            double* row = O.row(i);
            int32_t* st = nst ? O.st(i) : nullptr;
            const ObjIn in = B.object(i, s, n, true);
            LCFE_PT(5);
            const int rc = RunSet<W, SET, CAP>::run(in, ws, row, st);
            if constexpr (SetTraits<SET>::overflow_list >= 0) {
                // (research: r band longer than the Mexican-hat grid of this tier) the long-object tier takes the light curve
                if (rc == -100 && threadIdx.x == 0) bins.append(SetTraits<SET>::overflow_list, (int)i);
            }
            (void)rc;
            LCFE_PT0B();
        }
    }
    nan_fill_bins<W>(bins, 0, nan_from, O, ncol, nst);
    LCFE_PT(5);
    LCFE_PT_FLUSH();
}

// Statistics, lean layout (stat_lean.hpp) for the tiers up to 512 rows.  Same ticket scheme as
// set_kernel; an object that does not fit the lean shape is appended to the fallback list, which a
// set_kernel<SET_STAT, CAP> launch processes afterwards.
// waves per SIMD the LDS footprint allows (5.6 / 9.9 / 18.4 KiB per object): the register budget follows
template <int CAP> struct stat_lean_waves { static constexpr int N = (CAP <= 128) ? 4 : ((CAP <= 256) ? 3 : 2); };

template <int CAP>
__global__ __launch_bounds__(64, stat_lean_waves<CAP>::N) void stat_lean_kernel(BatchView B, Bins bins, int bin, SetOut O,
                                                       unsigned long long* ticket, int chunk) {
    __shared__ StatLeanLds<CAP> L;
    __shared__ long long next_ticket;
    using W = WaveDev;
    const int count = bins.count(bin);
    const int* list = bins.list(bin);
    // tickets of at least two light curves: one counter serves about 90 tickets per microsecond, which a statistics
    // tier of 20 000 light curves would otherwise spend more time on than on the light curves
    chunk = ticket_chunk(count, chunk, 2, 2);
    LCFE_PT_INIT();
    LCFE_PT0();
    for (;;) {
        const int64_t base = block_ticket(ticket, next_ticket) * chunk;
        if (base >= count) break;
        const int nk = (count - base < chunk) ? (int)(count - base) : chunk;
        TicketChunk tc;
        tc.load(list, base, nk, B);
        for (int k = 0; k < nk; ++k) {
            const auto [obj, s, n] = tc.object(k);
            const ObjIn in = B.object(obj, s, n, false);
            LCFE_PT(5);
            const bool lean = stat_lean_stage<CAP>(in, L);
            LCFE_PT(0);
            if (lean) {
                stat_lean_object<CAP>((int)n, L);
                LCFE_PT0B();
                store_row<W>(L.out, O.row(obj), STAT_NCOL);
                W::sync();
                LCFE_PT(3);
            } else if (threadIdx.x == 0) bins.append(kStatFallbackList, (int)obj);
        }
    }
    LCFE_PT(5);
    LCFE_PT_FLUSH();
}

// ---------------------------------------------------------------------------------------------------------------
// The long-object tier.  The reference has no limit on the rows of a light curve; the LDS tiers end at 2048 rows
// (1024 for the object-level fits and the research set).  Longer light curves -- and the ones that overflow a per-band
// limit of the LDS tiers -- run through the SAME templates with CAP = kLongCap, their working set (the structures that
// are LDS in the tiers) in a per-workgroup slab of global scratch: one wavefront per workgroup, a handful of workgroups
// (such objects are rare; the reference's own loaders truncate light curves at 300-500 points).  Up to three index
// lists are drained through one ticket counter.  Light curves beyond kLongCap rows keep NaN and status -100.
constexpr int kLongCap = 16384;
constexpr int kLongGrid = 16;
template <int SET> constexpr size_t long_slab_bytes() { return (sizeof(SetLds<SET, kLongCap>) + 255) & ~(size_t)255; }

template <int SET>
__global__ __launch_bounds__(64) void set_long_kernel(BatchView B, Bins bins, int l0, int l1, int l2, SetOut O,
                                                      unsigned long long* ticket, char* slabs) {
    using W = LongDev;
    __shared__ long long next_ticket;
    SetLds<SET, kLongCap>& ws = *reinterpret_cast<SetLds<SET, kLongCap>*>(slabs + (size_t)blockIdx.x * long_slab_bytes<SET>());
    const int ncol = SetTraits<SET>::ncols, nst = SetTraits<SET>::nstatus;
    const int c0 = (l0 >= 0) ? bins.count(l0) : 0, c1 = (l1 >= 0) ? bins.count(l1) : 0, c2 = (l2 >= 0) ? bins.count(l2) : 0;
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= (int64_t)c0 + c1 + c2) break;
        const int li = (pos < c0) ? l0 : ((pos < (int64_t)c0 + c1) ? l1 : l2);
        const int64_t at = (pos < c0) ? pos : ((pos < (int64_t)c0 + c1) ? pos - c0 : pos - c0 - c1);
        const auto [i, s, n] = take_object(B, bins.list(li), at);
        double* row = O.row(i);
        int32_t* st = nst ? O.st(i) : nullptr;
        if (n <= kLongCap) {
            const ObjIn in = B.object(i, s, n, true);
            RunSet<W, SET, kLongCap>::run(in, ws, row, st);
        } else {
            // (O.unavailable spelled out on the two addresses above: rebuilt from i and the view in this branch they
            //  cost set_long_kernel<9>, <12> two or three VGPRs and <2>, at 255 VGPRs, two AGPRs)
            fill_row_nan<W>(row, ncol);
            if (st) for (int k = threadIdx.x; k < nst; k += 64) st[k] = -100;
        }
        __syncthreads();
    }
}

// (the set's eighth ticket counter; the callers have checked that the workspace holds the slabs)
template <int SET>
int SetLaunch::long_tier(int l0, int l1, int l2) const {
    hipLaunchKernelGGL(set_long_kernel<SET>, dim3(kLongGrid), dim3(64), 0, stream, B, bins, l0, l1, l2, O,
                       tickets + SetTraits<SET>::ticket_base + 7, long_slabs);
    HIP_TRY(hipGetLastError());
    return 0;
}

// Statistics, several light curves per wavefront and the bands in lanes of their own (stat_lanes.hpp: LPO = lanes per
// light curve, CAP = rows a lane holds -- a band of P parts has up to P x CAP, ITERS = rows / LPO of the light curve).
// One workgroup = one batch of 64 / LPO consecutive entries of one of the lists stat_plan_kernel fills; the routes are
// served in the table's order, the long batches first: they are the ones whose tail would otherwise stick out.
struct StatLanesRoute {
    int list, lpo, cap, iters;
    constexpr int batch() const { return 64 / lpo; }       // light curves per workgroup
    constexpr int rows() const { return lpo * iters; }      // rows of a light curve
    // what stat_plan_kernel calls `eff`: the rows of u a lane group takes (r and i twice that, g, z, y the same: asserted below)
    constexpr int eff() const { return (lpo == 8) ? lanes_capacity<LanesLayout<8>>(0, cap) : lanes_capacity<LanesLayout<16>>(0, cap); }
};
constexpr int kStatLanesRoutes = 5;
constexpr StatLanesRoute kStatLanesRoute[kStatLanesRoutes] = {
    {kStatW32List, 16, 32, 32}, {kStatW16List, 16, 32, 16}, {kStatL32xList, 8, 32, 32}, {kStatL32List, 8, 32, 16}, {kStatL16List, 8, 16, 16}};
template <class L>
constexpr bool lanes_eff_proportions() {
    for (int b = 0; b < kLanesBands; ++b)
        if (L::parts(b) != ((b == 2 || b == 3) ? 2 : 1) * L::parts(0)) return false;
    return true;
}
static_assert(lanes_eff_proportions<LanesLayout<8>>() && lanes_eff_proportions<LanesLayout<16>>(), "r and i take twice the rows of the other bands");
constexpr int kStatLanesMaxCap = 32;                        // the LDS buffer of the kernel
// does the kernel behind `list` take every light curve of up to n rows whose bands need up to `eff` rows per lane of 8?
constexpr bool stat_route_takes(int list, int n, int eff) {
    for (int r = 0; r < kStatLanesRoutes; ++r)
        if (kStatLanesRoute[r].list == list)
            return kStatLanesRoute[r].cap <= kStatLanesMaxCap && n <= kStatLanesRoute[r].rows() && eff <= kStatLanesRoute[r].eff();
    return false;
}
// The lists' lengths are known on the device only; the grid covers n_obj / 4 + 6 batches and the workgroups behind the
// last batch leave at once.  A light curve whose rows turn out not to ascend in time is appended to list `retry`.
// Batch `b`, numbered from route R's first: route R's if its list has that many batches, else the next route's.
template <int R>
__device__ __forceinline__ void stat_lanes_route(int b, const int (&count)[kStatLanesRoutes], const BatchView& B, const Bins& bins, LanesBuf lbuf,
                                                 LanesBuf lall, const SetOut& O, int retry) {
    if constexpr (R < kStatLanesRoutes) {
        constexpr StatLanesRoute r = kStatLanesRoute[R];
        const int nb = (count[R] + r.batch() - 1) / r.batch();
        if (b < nb) {
            stat_lanes_run<r.lpo, r.cap, r.iters>(B.offsets, B.t, B.f, B.e, B.b, bins.list(r.list), count[R], b, lbuf, lall, O, bins, retry);
            return;
        }
        stat_lanes_route<R + 1>(b - nb, count, B, bins, lbuf, lall, O, retry);
    }
}
#ifdef LCFE_DEBUG
constexpr double kLanesCanary = 0x1.5ca1ab1edeadp+900;
#endif
__global__ __launch_bounds__(64, 2) void stat_lanes_all_kernel(BatchView B, Bins bins, int retry, SetOut O) {
#ifdef LCFE_DEBUG
    // debug build: canary words around the buffers, verified when the workgroup's batch is done
    struct Framed { double pre[8]; StatLanesLds<kStatLanesMaxCap> L; double post[8]; };
    __shared__ Framed F;
    StatLanesLds<kStatLanesMaxCap>& L = F.L;
    if (threadIdx.x < 8) { F.pre[threadIdx.x] = kLanesCanary; F.post[threadIdx.x] = kLanesCanary; }
    __syncthreads();
    unsigned int lanes_bad[2] = {0u, 0u};
    struct CanaryCheck {
        Framed& F;
        unsigned int (&bad)[2];
        __device__ ~CanaryCheck() {
            __syncthreads();
            if (threadIdx.x < 8 && (F.pre[threadIdx.x] != kLanesCanary || F.post[threadIdx.x] != kLanesCanary)) atomicAdd(&g_lanes_check[1], 1u);
            if (bad[0]) { atomicAdd(&g_lanes_check[0], bad[0]); g_lanes_check[2] = bad[1]; }
        }
    } canary_check{F, lanes_bad};
    unsigned int* const bad_p = lanes_bad;
#else
    __shared__ StatLanesLds<kStatLanesMaxCap> L;
    unsigned int* const bad_p = nullptr;
#endif
    const LanesBuf lbuf = lanes_buf(L.buf, 64 * StatLanesLds<kStatLanesMaxCap>::STRIDE, bad_p), lall = lanes_buf(L.all_rows, 8 * 17, bad_p);
    static_assert(kStatLanesRoutes == 5, "one count per route");
    const int count[kStatLanesRoutes] = {bins.count(kStatLanesRoute[0].list), bins.count(kStatLanesRoute[1].list),
                                         bins.count(kStatLanesRoute[2].list), bins.count(kStatLanesRoute[3].list),
                                         bins.count(kStatLanesRoute[4].list)};
    stat_lanes_route<0>((int)blockIdx.x, count, B, bins, lbuf, lall, O, retry);
}

// Which statistics kernel takes a light curve of up to 512 rows: ONE launch over the three tier lists (128 / 256 / 512
// rows), 8 lanes per light curve count its rows per band (1 byte per row is read, once) and the light curve is appended
// to the list of the cheapest lanes variant its bands fit:
//     rows <= 128   bands <= 16 rows (r, i: 32)   -> kStatL16List   (8 lanes per light curve, 16-row lanes)
//     rows <= 128   bands <= 32 (64)              -> kStatL32List   (8 lanes, 32-row lanes)
//     rows <= 256   bands <= 32 (64)              -> kStatL32xList  (8 lanes, 32-row lanes, 32 rows per lane loaded)
//     rows <= 256   bands <= 64 (128)             -> kStatW16List   (16 lanes per light curve)
//     rows <= 512   bands <= 64 (128)             -> kStatW32List   (16 lanes per light curve)
//     anything else (longer bands, unknown band codes, no rows)     -> kStatRetryList (one light curve per wavefront)
// The lists are private to the statistics set: the tier lists every other set reads are never appended to.  A workgroup
// takes 128 consecutive entries of one tier list (the long tier first); the lists' lengths are known on the device only,
// so the grid covers n_obj / 128 + 3 workgroups and the ones behind the last slice leave at once.  Lists are appended
// per workgroup with one atomic per destination.
// (stat_plan_kernel's thresholds, written once more here and held against the route table and the lanes layouts: a
//  route or layout that no longer takes what the plan sends it fails the build.  The kernel below has literals of its
//  own, which nothing ties to these: whoever edits them edits this list with them -- else a light curve reaches a list
//  whose kernel can only send it on to the retry list.)
static_assert(stat_route_takes(kStatL16List, 128, 16) && stat_route_takes(kStatL32List, 128, 32) && stat_route_takes(kStatW16List, 128, 64) &&
                  stat_route_takes(kStatL32xList, 256, 32) && stat_route_takes(kStatW16List, 256, 64) && stat_route_takes(kStatW32List, 512, 64),
              "stat_plan_kernel's thresholds (eff <= 16 / 32 / 64, n <= 128 / 256 / 512) and kStatLanesRoute");
constexpr int kPlanThreads = 1024;
constexpr int kPlanDst = 6;
template <int ITERS>
__device__ __forceinline__ unsigned long long stat_plan_count(const uint8_t* pb, int n, int j, bool& known) {
    // ITERS rows per lane, all loads in flight at once
    int bb[ITERS];
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int row = it * 8 + j;
        bb[it] = (row < n) ? (int)pb[row] : 256;
    }
    // rows per band: six 10-bit counters in one 64-bit word per lane (codes above 5 count in the bits that fall off)
    unsigned long long acc = 0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        const int b = bb[it];
        known = known && (b < 6 || b == 256);
        acc += 1ull << (10 * ((b < 6) ? b : 6));
    }
    return acc;
}

__global__ __launch_bounds__(kPlanThreads) void stat_plan_kernel(BatchView B, Bins bins) {
    __shared__ int wcount[kPlanThreads / 64][kPlanDst];
    __shared__ int base[kPlanDst];
    constexpr int PER = kPlanThreads / 8;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, g = lane >> 3, j = lane & 7;
    const int c0 = bins.count(0), c1 = bins.count(1), c2 = bins.count(2);
    const int nb2 = (c2 + PER - 1) / PER, nb1 = (c1 + PER - 1) / PER, nb0 = (c0 + PER - 1) / PER;
    int blk = (int)blockIdx.x, tier, count;
    if (blk < nb2) { tier = 2; count = c2; }
    else if (blk < nb2 + nb1) { tier = 1; count = c1; blk -= nb2; }
    else if (blk < nb2 + nb1 + nb0) { tier = 0; count = c0; blk -= nb2 + nb1; }
    else return;
    const int64_t pos = (int64_t)blk * PER + wave * 8 + g;
    int obj = -1, n = 0;
    int64_t s0 = 0;
    if (pos < count) {
        obj = bins.list(tier)[pos];
        s0 = B.offsets[obj];
        n = (int)(B.offsets[obj + 1] - s0);
    }
    bool known = true;
    unsigned long long acc;
    if (tier == 0) acc = stat_plan_count<16>(B.b + s0, n, j, known);
    else if (tier == 1) acc = stat_plan_count<32>(B.b + s0, n, j, known);
    else acc = stat_plan_count<64>(B.b + s0, n, j, known);
    acc = GroupDev<8>::reduce((long long)acc, [](long long x, long long y) { return x + y; });
    int cnt[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) cnt[k] = (int)(acc >> (10 * k)) & 1023;
    known = GroupDev<8>::all(known);
    // what a lane of an 8-lane group must hold: the rows of u, g, z, y and half the rows of r, i
    int eff = cnt[0];
    eff = (cnt[1] > eff) ? cnt[1] : eff;
    eff = (cnt[4] > eff) ? cnt[4] : eff;
    eff = (cnt[5] > eff) ? cnt[5] : eff;
    eff = ((cnt[2] + 1) / 2 > eff) ? (cnt[2] + 1) / 2 : eff;
    eff = ((cnt[3] + 1) / 2 > eff) ? (cnt[3] + 1) / 2 : eff;
    const bool fits = known && n >= 1 && n <= 512;
    int cls = -1;
    if (obj >= 0 && j == 0) {
        cls = 5;
        if (fits && eff <= 64) {
            if (n <= 128) cls = (eff <= 16) ? 0 : ((eff <= 32) ? 1 : 3);
            else if (n <= 256) cls = (eff <= 32) ? 2 : 3;
            else cls = 4;
        }
    }
    int rank = 0;
#pragma unroll
    for (int c = 0; c < kPlanDst; ++c) {
        const unsigned long long m = __ballot(cls == c);
        if (cls == c) rank = WaveDev::prefix(m);
        if (lane == 0) wcount[wave][c] = popcll(m);
    }
    __syncthreads();
    auto dst_of = [](int c) { return (c == 0) ? kStatL16List : (c == 1) ? kStatL32List : (c == 2) ? kStatL32xList : (c == 3) ? kStatW16List : (c == 4) ? kStatW32List : kStatRetryList; };
    if (threadIdx.x < kPlanDst) {
        int total = 0;
        for (int w = 0; w < kPlanThreads / 64; ++w) {
            const int c = wcount[w][threadIdx.x];
            wcount[w][threadIdx.x] = total;
            total += c;
        }
        base[threadIdx.x] = total ? bins.reserve(dst_of((int)threadIdx.x), total) : 0;
    }
    __syncthreads();
    if (cls >= 0) bins.list(dst_of(cls))[base[cls] + wcount[wave][cls] + rank] = obj;
}

// ---------------------------------------------------------------------------------------------------------------
// Bazin fits, fit by fit.  With one object per wavefront the six band fits of a light curve run side by side in
// 8-lane groups, but TRF's evaluation count is heavy-tailed (median 26, p99 556, cap 2000): the wave lasts as long as
// its slowest band and the other groups idle -- 37 % of the lane-group time did useful work.  Here the unit of work is
// ONE FIT: a partition pass writes every object's band-partitioned, time-sorted rows to global scratch and appends its
// fits to a list per band-length tier; the fit kernel runs a flat loop in which every 8-lane group advances the solver
// of its own fit by one phase per trip (trf.hpp: trf_outer / trf_inner) and takes the next fit from a device-side
// ticket counter the moment its own is finished -- the groups of a wave never wait for each other.  The arithmetic of
// a fit is exactly that of bazin_fit_band; only the schedule differs.
//
// Bands of up to 16 rows (tier 0) run on 4-lane groups, sixteen fits per wavefront: the trust-region algebra of a fit is
// wave-uniform scalar work that every lane of its group repeats, so a group of half the width halves it per fit, and
// wave.hpp's virtual lanes keep every sum in the order of the 8-lane group -- the results are bit-identical.  Tier 0 has
// no launch of its own: the kernel of the 32-row tier serves both lists (see bazin_fit_kernel).
// (The tiers -- rows, lanes per fit, groups per wave, register budgets, which tier hosts which -- and fit_tier_of, the
// tier of a band of m rows: fit_tier_table.hpp.  The count and ticket slots of the lists: workspace.hpp.)
struct FitWs {
    double* pt;            // band-partitioned copies of t / flux / err, indexed like the CSR arrays
    double* pf;
    double* pe;
    int* pboff;            // [n_obj][8] band offsets inside the object's slice
    int* fits;             // [kFitTiers][6 n_obj] fit ids (object * 8 + band)
    int64_t fit_stride;
};

// (times and fluxes are read from the partition pass's copy in global memory -- L2-resident, 16 bytes per row and
//  evaluation -- instead of a copy in LDS: 2.5 KB per fit at 32 rows instead of 3 KB = eight wavefronts per CU where six fitted)
template <int BCAP>
struct FitRegion {
    double r[BCAP], rn[BCAP], w[BCAP];     // rn doubles as the key scratch of the median before the first trial point
    double A[6][BCAP + 5];
    double slot[2];
    __device__ __forceinline__ double* trial() { return rn; }
    __device__ __forceinline__ double* median_slot() { return slot; }
};
// The 16-row tier: sixteen of these must fit where eight FitRegion<32> do (20 KiB per wavefront, eight wavefronts per
// CU), so two arrays share storage with matrix columns that are dead while they live.  The residual at the trial point
// lies in the residual column A[5]: that column is written by trf_outer (from r) and last read when the QR hands over
// Q^T f, the trial residual is written after that and copied to r before the next trf_outer.  The two words of the median
// lie in A[4], which nothing uses before the first Jacobian.
struct FitRegionNarrow {
    double r[kFitNarrowRows], w[kFitNarrowRows];
    double A[6][kFitNarrowRows + 5];
    __device__ __forceinline__ double* trial() { return A[5]; }
    __device__ __forceinline__ double* median_slot() { return A[4]; }
};
static_assert(kFitNarrowGroups * sizeof(FitRegionNarrow) <= kFitTierTable[kFitNarrowHost].groups * sizeof(FitRegion<fit_tier_cap(kFitNarrowHost)>),
              "the narrow regions fit the LDS of their host tier");

// partition pass: one object per wavefront (tier lists of the feature sets), up to `chunk` objects per ticket
template <int CAP>
__global__ __launch_bounds__(64, 2) void bazin_partition_kernel(BatchView B, Bins bins, int bin, int nan_from, FitWs F, SetOut O,
                                                                unsigned long long* ticket, int chunk, int narrow) {
    __shared__ ObjLds<CAP> L;
    __shared__ long long next_ticket;
    __shared__ int loc[kFitTiers][64], nloc[kFitTiers], base_of[kFitTiers];
    using W = WaveDev;
    const int count = bins.count(bin);
    const int* list = bins.list(bin);
    chunk = ticket_chunk(count, chunk, 4, 1);
    for (;;) {
        if (threadIdx.x == 0) for (int q = 0; q < kFitTiers; ++q) nloc[q] = 0;
        const int64_t base = block_ticket(ticket, next_ticket) * chunk;
        if (base >= count) break;
        const int nk = (count - base < chunk) ? (int)(count - base) : chunk;
        for (int k = 0; k < nk; ++k) {
            const int64_t i = list[base + k];
            const int64_t s = B.offsets[i];
            const int n = (int)(B.offsets[i + 1] - s);
            const ObjIn in = B.object(i, s, n, false);
            stage_object<W, CAP>(in, L);
            const int nb = L.boff[6];
            for (int q = threadIdx.x; q < nb; q += 64) { F.pt[s + q] = L.bt[q]; F.pf[s + q] = L.bf[q]; F.pe[s + q] = L.be[q]; }
            if (threadIdx.x < 8) F.pboff[i * 8 + threadIdx.x] = L.boff[threadIdx.x];
            int mb = 0;
#pragma unroll
            for (int b = 0; b < 6; ++b) { const int m = L.boff[b + 1] - L.boff[b]; mb = (m > mb) ? m : mb; }
            if (mb > kFitMaxRows) {
                // a band beyond the largest fit tier: the whole object goes to the object-level kernel, which takes
                // light curves of up to 1024 rows; beyond that the fit is not available (NaN, status -100)
                if (n <= kFitObjectRows) {
                    if (threadIdx.x == 0) bins.append(kBazinFallbackList, (int)i);
                } else {
                    // the long-object tier takes it (when the caller's workspace has its slabs); NaN and -100 until then
                    O.unavailable<W>(i, BAZIN_NCOL, SetTraits<SET_BAZIN>::nstatus);
                    if (threadIdx.x == 0) bins.append(kBazinLongList, (int)i);
                }
            } else if (threadIdx.x < 6) {
                const int b = threadIdx.x;
                const int m = L.boff[b + 1] - L.boff[b];
                if (m < 5) {                                                    // bazin_fitting.py:76-87
                    double* o8 = O.row(i) + 8 * b;
                    for (int q = 0; q < 8; ++q) o8[q] = qnan();
                    if (int32_t* st = O.st(i)) { st[2 * b] = TRF_FAIL_TOO_FEW; st[2 * b + 1] = 0; }
                } else {
                    const int tier = fit_tier_of(m, narrow);
                    const int slot = atomicAdd(&nloc[tier], 1);                 // LDS atomic: order inside a chunk is free
                    if (slot < 64) loc[tier][slot] = (int)i * 8 + b;
                }
            }
            __syncthreads();
        }
        // one global atomic per tier and chunk
        if (threadIdx.x < kFitTiers) base_of[threadIdx.x] = nloc[threadIdx.x] ? atomicAdd(&bins.counts[kFitCountBase + threadIdx.x], nloc[threadIdx.x]) : 0;
        __syncthreads();
        for (int tr = 0; tr < kFitTiers; ++tr)
            for (int q = threadIdx.x; q < nloc[tr] && q < 64; q += 64)
                if (base_of[tr] + q < F.fit_stride) F.fits[tr * F.fit_stride + base_of[tr] + q] = loc[tr][q];
        __syncthreads();
    }
    nan_fill_bins<W>(bins, 0, nan_from, O, BAZIN_NCOL, SetTraits<SET_BAZIN>::nstatus);
}

enum { FIT_IDLE = 3, FIT_EXIT = 4 };      // beside TRF_PH_OUTER / INNER / DONE

// Blocks of a kernel that serves the 16-row list (4-lane groups) and the 32-row list (8-lane groups): the first
// fit_narrow_first_blocks() blocks start on the 16-row list, the others on the 32-row list, and every block goes on to
// the other list when the tickets of its own run out -- no block waits while either list has fits left, whatever the
// split.  The split follows the work: a fit on a 4-lane group costs about 9/16 of one on an 8-lane group.
__device__ __forceinline__ int fit_narrow_first_blocks(int count_narrow, int count_wide) {
    const long long wn = 9ll * count_narrow, ww = 16ll * count_wide;
    return (wn + ww > 0) ? (int)(((long long)gridDim.x * wn + (wn + ww) / 2) / (wn + ww)) : 0;
}

// the flat loop of one list: G = lane group of one fit, NG groups of the wave take fits, Region = their LDS regions
template <class G, int NG, class Region>
__device__ __forceinline__ void bazin_fit_loop(Region* R, const BatchView& B, const FitWs& F, const int* list, int count, const SetOut& O,
                                               unsigned long long* ticket) {
    static_assert(NG <= G::NGROUPS, "one region per lane group");
    Region& Rg = R[(G::group_id() < NG) ? G::group_id() : 0];
    TrfView<5> V;
#pragma unroll
    for (int k = 0; k < 6; ++k) V.A[k] = Rg.A[k];
    V.r = Rg.r; V.rn = Rg.trial(); V.w = Rg.w;
    const int gl = G::lane();
    const int leader = (int)(threadIdx.x & 63) & ~(G::LANES - 1);
    TrfState<5> Z;
    Z.phase = (G::group_id() < NG) ? FIT_IDLE : FIT_EXIT;
    int m = 0;
    int64_t obj = 0, src = 0;
    int band = 0;
    for (;;) {
        if (Z.phase == FIT_IDLE) {
            int tk = 0;
            if (gl == 0) tk = (int)atomicAdd(ticket, 1ull);
            tk = __shfl(tk, leader, 64);
            if (tk >= count) Z.phase = FIT_EXIT;
            else {
                const int id = list[tk];
                obj = id >> 3;
                band = id & 7;
                const int b0 = F.pboff[obj * 8 + band];
                m = F.pboff[obj * 8 + band + 1] - b0;
                src = B.offsets[obj] + b0;
                bazin_prepare<G, TrfView<5>>(F.pt + src, F.pf + src, F.pe + src, m, V, Rg.median_slot(), reinterpret_cast<unsigned long long*>(Rg.trial()), Z);
                trf_begin<G, BazinModel, TrfView<5>>(BazinModel(), F.pt + src, F.pf + src, m, Z, V);
            }
        }
        if (__ballot(Z.phase != FIT_EXIT) == 0ull) break;
        if (Z.phase == TRF_PH_OUTER) trf_outer<G, BazinModel, TrfView<5>>(m, Z, V);
        if (Z.phase == TRF_PH_INNER) trf_inner<G, BazinModel, TrfView<5>>(BazinModel(), F.pt + src, F.pf + src, m, Z, V);
        if (Z.phase == TRF_PH_DONE) {
            bazin_finish<G>(F.pt + src, F.pf + src, F.pe + src, m, Z, O.row(obj) + 8 * band);
            int32_t* st = O.st(obj);
            if (st && gl == 0) {
                st[2 * band] = Z.res.status;
                st[2 * band + 1] = Z.res.nfev;
            }
            G::sync();
            Z.phase = FIT_IDLE;
        }
    }
}

// list `tier` (bands of up to BCAP rows); the 32-row kernel also serves list 0 (up to 16 rows, 4-lane groups): a kernel
// of its own behind the other four would add its longest fit to the end of the fit stream
template <int BCAP>
__global__ __launch_bounds__(64, (fit_tier_row(BCAP).waves_bazin)) void bazin_fit_kernel(BatchView B, Bins bins, FitWs F, int tier, SetOut O,
                                                            unsigned long long* ticket, unsigned long long* ticket_narrow) {
    constexpr FitTierRow T = fit_tier_row(BCAP);
    static_assert(T.id >= 0 && T.kernel, "a tier of fit_tier_table.hpp with kernels of its own");
    constexpr int NG = T.groups;
    const int count = bins.counts[kFitCountBase + tier];
    const int* list = F.fits + (int64_t)tier * F.fit_stride;
    if constexpr (T.id == kFitNarrowHost) {
        __shared__ union Lds { FitRegion<BCAP> wide[NG]; FitRegionNarrow narrow[kFitNarrowGroups]; __device__ Lds() {} } R;
        const int count_n = bins.counts[kFitCountBase + kFitNarrowTier];
        const int* list_n = F.fits + (int64_t)kFitNarrowTier * F.fit_stride;
        const bool narrow_first = (int)blockIdx.x < fit_narrow_first_blocks(count_n, count);
        for (int pass = 0; pass < 2; ++pass) {
            if ((pass == 0) == narrow_first) {
                if (count_n > 0) bazin_fit_loop<GroupDev<kFitNarrowLanes>, kFitNarrowGroups>(R.narrow, B, F, list_n, count_n, O, ticket_narrow);
            } else {
                if (count > 0) bazin_fit_loop<GroupDev<T.lanes>, NG>(R.wide, B, F, list, count, O, ticket);
            }
            __syncthreads();
        }
    } else {
        __shared__ FitRegion<BCAP> R[NG];
        bazin_fit_loop<GroupDev<T.lanes>, NG>(R, B, F, list, count, O, ticket);
    }
}

// the four cross-band columns of every object (bazin_fitting.py:217-249) once all its fits are in
__global__ __launch_bounds__(256) void bazin_cross_kernel(BatchView B, SetOut O) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= B.n_obj) return;
    double o[BAZIN_NCOL];
    double* row = O.row(i);
    for (int k = 0; k < 48; ++k) o[k] = row[k];
    bazin_cross_band(o);
    for (int k = 48; k < 52; ++k) row[k] = o[k];
}

// ---------------------------------------------------------------------------------------------------------------
// Decline-model fits (v55 power-law set), fit by fit: same scheme as the Bazin fits above.  A partition pass writes,
// per object and band g/r/i, the post-peak rows (times relative to the peak, fluxes) and their peak flux and total
// sum of squares, and queues the band's nine fits: the seven power laws (two parameters, the exponent is data) in
// list A, the exponential and the linear model (three parameters) in list B, per tier of the post-peak row count.
struct PlWs {
    double* tp;            // post-peak times of band j of object i at offsets[i] + boff[j + 1] ..., indexed like the CSR arrays
    double* fp;
    double* peak;          // [n_obj][3]
    double* sstot;         // [n_obj][3]
    int* pboff;            // [n_obj][8]
    int* kk;               // [n_obj][3] post-peak rows (-1: no fits)
    int* fitsA;            // [kFitTiers][21 n_obj]   ids: object * 32 + band * 9 + model
    int* fitsB;            // [kFitTiers][6 n_obj]
    int64_t strideA, strideB;
};

// (the decline fits keep their rows in LDS: read from global memory their 32-row tiers ran 3-5 % slower -- LDS is not
//  what limits their occupancy)
template <int N, int BCAP>
struct PlRegion {
    double t[BCAP], f[BCAP];
    double r[BCAP], rn[BCAP], w[BCAP];
    double A[N + 1][BCAP + N];
};

template <int CAP>
__global__ __launch_bounds__(64, 2) void powerlaw_partition_kernel(BatchView B, Bins bins, int bin, int nan_from, PlWs F, SetOut O,
                                                                   unsigned long long* ticket, int chunk, int narrow) {
    __shared__ ObjLds<CAP> L;
    __shared__ long long next_ticket;
    using W = WaveDev;
    const int count = bins.count(bin);
    const int* list = bins.list(bin);
    chunk = ticket_chunk(count, chunk, 4, 1);
    for (;;) {
        const int64_t base = block_ticket(ticket, next_ticket) * chunk;
        if (base >= count) break;
        const int nk = (count - base < chunk) ? (int)(count - base) : chunk;
        for (int q = 0; q < nk; ++q) {
            const int64_t i = list[base + q];
            const int64_t s = B.offsets[i];
            const int n = (int)(B.offsets[i + 1] - s);
            const ObjIn in = B.object(i, s, n, false);
            stage_object<W, CAP>(in, L);
            if (threadIdx.x < 8) F.pboff[i * 8 + threadIdx.x] = L.boff[threadIdx.x];
            int kb[3];
            for (int j = 0; j < 3; ++j) {
                const int b0 = L.boff[j + 1], m = L.boff[j + 2] - b0;
                int k, first;
                double peak_flux, ss_tot;
                powerlaw_band_prepare<W>(L.bt + b0, L.bf + b0, m, F.tp + s + b0, F.fp + s + b0, k, first, peak_flux, ss_tot);
                kb[j] = k;
                if (threadIdx.x == 0) { F.kk[i * 3 + j] = k; F.peak[i * 3 + j] = peak_flux; F.sstot[i * 3 + j] = ss_tot; }
            }
            const int kmax = (kb[0] > kb[1]) ? ((kb[0] > kb[2]) ? kb[0] : kb[2]) : ((kb[1] > kb[2]) ? kb[1] : kb[2]);
            if (kmax > kFitMaxRows) {
                // more post-peak rows than the largest fit tier: object-level kernel (up to 1024 rows), else not available
                if (n <= kFitObjectRows) {
                    if (threadIdx.x == 0) bins.append(kPowerlawFallbackList, (int)i);
                } else {
                    O.unavailable<W>(i, POWERLAW_NCOL, SetTraits<SET_POWERLAW>::nstatus);
                    if (threadIdx.x == 0) bins.append(kPowerlawLongList, (int)i);
                }
            } else if (threadIdx.x < 3) {
                const int j = threadIdx.x;
                const int k = kb[j];
                if (k < 0) {                                                    // train_v55_powerlaw.py:150-151,162-163
                    double* o9 = O.row(i) + 9 * j;
                    int32_t* st = O.st(i);
                    for (int id = 0; id < 9; ++id) {
                        o9[id] = qnan();
                        if (st) { st[18 * j + 2 * id] = TRF_FAIL_TOO_FEW; st[18 * j + 2 * id + 1] = 0; }
                    }
                } else {
                    const int tier = fit_tier_of(k, narrow);
                    const int a0 = atomicAdd(&bins.counts[kPlCountA + tier], 7);
                    if (a0 + 7 <= F.strideA)
                        for (int id = 0; id < 7; ++id) F.fitsA[tier * F.strideA + a0 + id] = (int)i * 32 + j * 9 + id;
                    const int b0 = atomicAdd(&bins.counts[kPlCountB + tier], 2);
                    if (b0 + 2 <= F.strideB) {
                        F.fitsB[tier * F.strideB + b0] = (int)i * 32 + j * 9 + 7;
                        F.fitsB[tier * F.strideB + b0 + 1] = (int)i * 32 + j * 9 + 8;
                    }
                }
            }
            __syncthreads();
        }
    }
    nan_fill_bins<W>(bins, 0, nan_from, O, POWERLAW_NCOL, SetTraits<SET_POWERLAW>::nstatus);
}

// N = 2: the seven power laws (PowerModel, exponent from the fit id); N = 3: exponential and linear (Decline3Model)
template <int N> struct pl_model;
template <> struct pl_model<2> { using type = PowerModel; static __device__ __forceinline__ PowerModel make(int id) { return PowerModel{decline_exponent(id)}; } };
template <> struct pl_model<3> { using type = Decline3Model; static __device__ __forceinline__ Decline3Model make(int id) { return Decline3Model{id}; } };

template <class G, int N, int NG, class Region>
__device__ __forceinline__ void powerlaw_fit_loop(Region* R, const BatchView& B, const PlWs& F, const int* list, int count, const SetOut& O,
                                                  unsigned long long* ticket) {
    static_assert(NG <= G::NGROUPS, "one region per lane group");
    using M = typename pl_model<N>::type;
    Region& Rg = R[(G::group_id() < NG) ? G::group_id() : 0];
    TrfView<N> V;
#pragma unroll
    for (int k = 0; k <= N; ++k) V.A[k] = Rg.A[k];
    V.r = Rg.r; V.rn = Rg.rn; V.w = Rg.w;
    const int gl = G::lane();
    const int leader = (int)(threadIdx.x & 63) & ~(G::LANES - 1);
    TrfState<N> Z;
    Z.phase = (G::group_id() < NG) ? FIT_IDLE : FIT_EXIT;
    M model = pl_model<N>::make(N == 2 ? 0 : 7);
    int k = 0, id = 0, j = 0;
    int64_t obj = 0;
    double ss_tot = 0;
    for (;;) {
        if (Z.phase == FIT_IDLE) {
            int tk = 0;
            if (gl == 0) tk = (int)atomicAdd(ticket, 1ull);
            tk = __shfl(tk, leader, 64);
            if (tk >= count) Z.phase = FIT_EXIT;
            else {
                const int fid = list[tk];
                obj = fid >> 5;
                j = (fid & 31) / 9;
                id = (fid & 31) - 9 * j;
                k = F.kk[obj * 3 + j];
                ss_tot = F.sstot[obj * 3 + j];
                const int64_t src = B.offsets[obj] + F.pboff[obj * 8 + j + 1];
                for (int i = gl; i < k; i += G::LANES) { Rg.t[i] = F.tp[src + i]; Rg.f[i] = F.fp[src + i]; Rg.w[i] = 1.0; }
                model = pl_model<N>::make(id);
                decline_setup<N>(id, F.peak[obj * 3 + j], Z);
                G::sync();
                trf_begin<G, M, TrfView<N>>(model, Rg.t, Rg.f, k, Z, V);
            }
        }
        if (__ballot(Z.phase != FIT_EXIT) == 0ull) break;
        if (Z.phase == TRF_PH_OUTER) trf_outer<G, M, TrfView<N>>(k, Z, V);
        if (Z.phase == TRF_PH_INNER) trf_inner<G, M, TrfView<N>>(model, Rg.t, Rg.f, k, Z, V);
        if (Z.phase == TRF_PH_DONE) {
            decline_finish<G, M>(model, Rg.t, Rg.f, k, ss_tot, Z, O.row(obj) + 9 * j + id);
            int32_t* st = O.st(obj);
            if (st && gl == 0) {
                st[18 * j + 2 * id] = Z.res.status;
                st[18 * j + 2 * id + 1] = Z.res.nfev;
            }
            G::sync();
            Z.phase = FIT_IDLE;
        }
    }
}

// list `tier` of the N-parameter models; the 32-row kernel also serves list 0 on 4-lane groups (see bazin_fit_kernel)
template <int N, int BCAP>
__global__ __launch_bounds__(64, (fit_tier_row(BCAP).waves_decline)) void powerlaw_fit_kernel(BatchView B, Bins bins, PlWs F, int tier, SetOut O,
                                                                                  unsigned long long* ticket, unsigned long long* ticket_narrow) {
    constexpr FitTierRow T = fit_tier_row(BCAP);
    static_assert(T.id >= 0 && T.kernel, "a tier of fit_tier_table.hpp with kernels of its own");
    constexpr int NG = T.groups;
    constexpr int kCount = (N == 2) ? kPlCountA : kPlCountB;
    const int count = bins.counts[kCount + tier];
    const int* lists = (N == 2) ? F.fitsA : F.fitsB;
    const int64_t stride = (N == 2) ? F.strideA : F.strideB;
    const int* list = lists + (int64_t)tier * stride;
    if constexpr (T.id == kFitNarrowHost) {
        __shared__ union Lds { PlRegion<N, BCAP> wide[NG]; PlRegion<N, kFitNarrowRows> narrow[kFitNarrowGroups]; __device__ Lds() {} } R;
        const int count_n = bins.counts[kCount + kFitNarrowTier];
        const int* list_n = lists + (int64_t)kFitNarrowTier * stride;
        const bool narrow_first = (int)blockIdx.x < fit_narrow_first_blocks(count_n, count);
        for (int pass = 0; pass < 2; ++pass) {
            if ((pass == 0) == narrow_first) {
                if (count_n > 0) powerlaw_fit_loop<GroupDev<kFitNarrowLanes>, N, kFitNarrowGroups>(R.narrow, B, F, list_n, count_n, O, ticket_narrow);
            } else {
                if (count > 0) powerlaw_fit_loop<GroupDev<T.lanes>, N, NG>(R.wide, B, F, list, count, O, ticket);
            }
            __syncthreads();
        }
    } else {
        __shared__ PlRegion<N, BCAP> R[NG];
        powerlaw_fit_loop<GroupDev<T.lanes>, N, NG>(R, B, F, list, count, O, ticket);
    }
}

// ---- 2-D GP: one light curve per workgroup (256/512/1024 threads by tier); Gram matrix as 16x16
// lower-triangle tiles in LDS (NP <= 160) or, for longer light curves, in a per-workgroup slab of
// global scratch.  Objects come from the tier's index list through a ticket counter (one object per
// ticket: an L-BFGS-B run is 10^5..10^7 cycles and heavy-tailed).
template <int NP, bool GLOBAL_K>
__global__ __launch_bounds__(gp_threads<NP>::T, (gp_waves<NP>::N)) void gp_kernel(BatchView B, Bins bins, int bin, int nan_from, SetOut O,
                                                 double* kscratch, unsigned long long* ticket) {
    using Tier = GpTier<NP, GLOBAL_K>;
    using W = typename Tier::W;
    __shared__ typename Tier::Set S;
    __shared__ double Klds[Tier::kLdsDoubles];
    __shared__ long long next_ticket;
    double* Kg = kscratch + (size_t)blockIdx.x * (size_t)gp_store_doubles(NP);
    const int count = bins.count(gp_list(bin));
    const int* list = bins.list(gp_sorted_list(bin));      // longest first (gp_sort_kernel)
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= count) break;
        const auto [i, s, n64] = take_object(B, list, pos);
        double* row = O.row(i);
        int32_t* st = O.st(i);
        const ObjIn in = B.object(i, s, n64, false);
        gp_object<W, NP>(in, S, [&](const double* x, int n, double& f, double* g, bool need) {
            Tier::eval(S, Tier::matrix(Klds, Kg), x, n, f, g, need); }, st);
        store_row<W>(S.out, row, GP_NCOL);
        __syncthreads();
    }
    nan_fill_bins<W>(bins, 1, nan_from, O, GP_NCOL, 4);
}

// the same loop for the long-object tier (slabs: GpLongTier::kBytes)
__global__ __launch_bounds__(kGpLongThreads, 1) void gp_long_kernel(BatchView B, Bins bins, int bin, SetOut O, char* slabs,
                                                                   unsigned long long* ticket) {
    using Tier = GpLongTier;
    using W = Tier::W;
    constexpr int NP = kGpLongNP;
    __shared__ long long next_ticket;
    double* Kg = reinterpret_cast<double*>(slabs) + (size_t)blockIdx.x * (size_t)gp_store_doubles(NP);
    Tier::Set& S = *reinterpret_cast<Tier::Set*>(slabs + (size_t)kGpLongGrid * gp_store_doubles(NP) * 8 + (size_t)blockIdx.x * Tier::kSetBytes);
    const int count = bins.count(gp_list(bin));
    const int* list = bins.list(gp_list(bin));
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= count) break;
        const auto [i, s, n64] = take_object(B, list, pos);
        int32_t* st = O.st(i);
        const ObjIn in = B.object(i, s, n64, false);
        gp_object<W, NP>(in, S, [&](const double* x, int n, double& f, double* g, bool need) { Tier::eval(S, Kg, x, n, f, g, need); }, st);
        store_row<W>(S.out, O.row(i), GP_NCOL);
        __syncthreads();
    }
}

// ---- the 2-D GP's posterior on a caller's grid (lcfe_gp2d_grid_device): gp_kernel's loop with the grid
// stage as gp_object's tail, on each tier's own working set and matrix placement.  The outputs are the caller's arrays, one
// slice per light curve; a slice is NaN until the tail has written it.
struct GpGridOut {
    GpGridSpec G;
    const double* theta_in;            // [n_obj][4]; nullptr: fit mode
    double *mean, *var, *theta_out, *row27;
    int32_t* status;                   // [n_obj][GP_NSTATUS]
    // the column source of light curve i and where its columns start in mean and var
    using Src = GpGridSpec;
    static constexpr const char* kWorkspaceFn = "lcfe_gp2d_grid_workspace_bytes";
    __device__ __forceinline__ Src source(int64_t i, int64_t& base) const {
        base = i * G.size();
        return G;
    }
};
// ... and at a caller's points (lcfe_gp2d_points_device): light curve i has the columns q_off[i] .. q_off[i + 1] of q_t and
// q_lam, and of mean and var
struct GpPointsOut {
    const int64_t* q_off;              // [n_obj + 1]
    const double *q_t, *q_lam;
    int origin;
    const double* theta_in;
    double *mean, *var, *theta_out, *row27;
    int32_t* status;
    using Src = GpPointSpec;
    static constexpr const char* kWorkspaceFn = "lcfe_gp2d_points_workspace_bytes_for";
    __device__ __forceinline__ Src source(int64_t i, int64_t& base) const {
        base = q_off[i];
        return GpPointSpec{q_t + base, q_lam + base, (int)(q_off[i + 1] - base), origin};
    }
};

template <class Tier, int NP, class Out>
__device__ __forceinline__ void gp_grid_objects(const BatchView& B, const int* list, int count, const Out& O, typename Tier::Set& S,
                                                double* K, unsigned long long* ticket, long long& next_ticket) {
    using W = typename Tier::W;
    using KP = typename Tier::KPtr;
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= count) break;
        const ListObject o = take_object(B, list, pos);
        int64_t base;
        const typename Out::Src G = O.source(o.i, base);
        const int ng = G.size();
        double* mean = O.mean + base;
        double* var = O.var ? O.var + base : nullptr;
        double* th = O.theta_out + 4 * o.i;
        for (int g = W::lane(); g < ng; g += W::LANES) {
            mean[g] = qnan();
            if (var) var[g] = qnan();
        }
        if (W::lane() < 4) th[W::lane()] = qnan();
        const ObjIn in = B.object(o.i, o.s, o.n, false);
        const GpGridTail<KP, typename Out::Src> tail{O.theta_in != nullptr, G, (KP)K, O.theta_in ? O.theta_in + 4 * o.i : nullptr, th, mean, var};
        gp_object<W, NP>(in, S, [&](const double* x, int n, double& f, double* g, bool need) { Tier::eval(S, K, x, n, f, g, need); },
                         O.status + o.i * GP_NSTATUS, tail);
        if (O.row27) store_row<W>(S.out, O.row27 + o.i * GP_NCOL, GP_NCOL);
        __syncthreads();
    }
}

template <int NP, bool GLOBAL_K, class Out>
__global__ __launch_bounds__(gp_threads<NP>::T, (gp_waves<NP>::N)) void gp_grid_kernel(BatchView B, Bins bins, int bin, Out O,
                                                      double* kscratch, unsigned long long* ticket) {
    using Tier = GpTier<NP, GLOBAL_K, kGpGridUser>;
    __shared__ typename Tier::Set S;
    __shared__ double Klds[Tier::kLdsDoubles];
    __shared__ long long next_ticket;
    double* Kg = kscratch + (size_t)blockIdx.x * (size_t)gp_store_doubles(NP);
    gp_grid_objects<Tier, NP>(B, bins.list(gp_sorted_list(bin)), bins.count(gp_list(bin)), O, S, Tier::matrix(Klds, Kg), ticket, next_ticket);
}

// the long-object tier (slabs: GpLongTier::kBytes)
template <class Out>
__global__ __launch_bounds__(kGpLongThreads, 1) void gp_grid_long_kernel(BatchView B, Bins bins, int bin, Out O, char* slabs,
                                                                        unsigned long long* ticket) {
    using Tier = GpLongTierOf<kGpGridUser>;
    constexpr int NP = kGpLongNP;
    __shared__ long long next_ticket;
    double* Kg = reinterpret_cast<double*>(slabs) + (size_t)blockIdx.x * (size_t)gp_store_doubles(NP);
    typename Tier::Set& S = *reinterpret_cast<typename Tier::Set*>(slabs + (size_t)kGpLongGrid * gp_store_doubles(NP) * 8 + (size_t)blockIdx.x * Tier::kSetBytes);
    gp_grid_objects<Tier, NP>(B, bins.list(gp_list(bin)), bins.count(gp_list(bin)), O, S, Kg, ticket, next_ticket);
}

// The tickets of a GP tier are served longest light curve first: an evaluation costs ~N^3 and a run 10-100 evaluations, so
// in file order the last tickets of a tier can be its most expensive light curves (a 500-row one is 60 ms on ONE workgroup
// while the rest of the grid has drained; simulated on the bench shard, the 512-row tier ends 14 % after the ideal in file
// order and 2 % after it longest first).  One workgroup per tier: counting sort of the tier's list by row count into the
// tier's second list.  The order inside a row count is whatever the atomics give -- results do not depend on the order.
constexpr int kGpSortThreads = 1024;
__global__ __launch_bounds__(kGpSortThreads) void gp_sort_kernel(const int64_t* offsets, Bins bins) {
    const int tier = blockIdx.x;
    const int hi = gp_cap_of(tier);
    const int count = bins.count(gp_list(tier));
    const int* src = bins.list(gp_list(tier));
    int* dst = bins.list(gp_sorted_list(tier));
    __shared__ int hist[1024], wsum[kGpSortThreads / 64];
    hist[threadIdx.x] = 0;
    __syncthreads();
    for (int k = threadIdx.x; k < count; k += kGpSortThreads) {
        const int i = src[k];
        const int key = hi - (int)(offsets[i + 1] - offsets[i]);             // 0 = the longest light curve the tier takes
        atomicAdd(&hist[(key < 0) ? 0 : ((key > 1023) ? 1023 : key)], 1);
    }
    __syncthreads();
    // exclusive scan of the 1024 counters: inside the wavefronts, then over the 16 wavefront totals
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int mine = hist[threadIdx.x];
    int incl = mine;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int v = __shfl_up(incl, d, 64);
        if (lane >= d) incl += v;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    int before = 0;
    for (int w = 0; w < wave; ++w) before += wsum[w];
    __syncthreads();
    hist[threadIdx.x] = before + incl - mine;
    __syncthreads();
    for (int k = threadIdx.x; k < count; k += kGpSortThreads) {
        const int i = src[k];
        const int key = hi - (int)(offsets[i + 1] - offsets[i]);
        const int at = atomicAdd(&hist[(key < 0) ? 0 : ((key > 1023) ? 1023 : key)], 1);
        dst[at] = i;
    }
}

template <int NP, bool GLOBAL_K>
int SetLaunch::gp_tier(int ti, int nan_from, hipStream_t q, double* kscratch, int64_t cap) const {
    constexpr int kSlabs = gp_tier_row(NP).slabs;
    if (GLOBAL_K && (cap < 1 || cap > kSlabs)) cap = kSlabs;     // one slab of global scratch per workgroup
    {
        // tuning knob: LCFE_GP_GRID_<rows>=k caps the workgroups of a tier (fewer Gram matrices in flight = more of them in L2)
        char name[40];
        snprintf(name, sizeof name, "LCFE_GP_GRID_%d", NP);
        const char* e = getenv(name);
        if (e && atoi(e) > 0 && (cap < 1 || atoi(e) < cap)) cap = atoi(e);
    }
    return launch_grid(gp_kernel<NP, GLOBAL_K>, gp_threads<NP>::T, {0, cap}, B.n_obj, 1, q, dev, B, bins, ti, nan_from, O, kscratch,
                       tickets + SET_GP2D * 8 + ti);
}

// kslab[tier]: the tier's Gram-matrix slabs (WS_GP_TIER + tier; no bytes behind the pointer of a tier whose matrix is in LDS)
int SetLaunch::launch_gp(const hipStream_t* gs, int ngs, double* const* kslab) const {
    hipStream_t stream2 = gs[(ngs > 1) ? 1 : 0];
    // (A variant that keeps the matrix in the REGISTERS of the workgroup -- 2-D block-cyclic tiles,
    // register-tiled outer products -- was built and measured: slower on every tier, because hipcc
    // spends 412-512 registers per lane on the unrolled tile passes and spills at 1024 threads.)
    const int last = gp_last_tier(max_len);
    // every tier's list longest light curve first (on the first GP stream; the others wait for it)
    {
        hipLaunchKernelGGL(gp_sort_kernel, dim3((unsigned)(last + 1)), dim3(kGpSortThreads), 0, gs[0], B.offsets, bins);
        HIP_TRY(hipGetLastError());
        ++*n_launch;
        if (ngs > 1 && stream_wait(gs + 1, ngs - 1, gs[0])) return 1;
    }
    // Launch plan: which stream takes which tiers, in which order, and on how many workgroups at most.  Default (two GP
    // streams): longest tier first, tiers alternating between the streams -- the heavy-tailed end of one tier (single objects
    // of up to 50 ms) overlaps with the start of the next.  The 512-row tier holds a whole CU per workgroup (160 KB of LDS)
    // for the first half second of the step and is bound by the MFMA pipe: when the fit kernels run beside the GP (side
    // streams), 192 of the 256 CUs are enough for it and the other 64 let the fits overlap from the start -- +4.5 % light
    // curves/s for the whole step (75.2 k against 72.0 k, two runs each), where the GP on its own would lose 12 %.
    // LCFE_GP_PLAN overrides it for experiments: streams separated by '|', tiers (0 = 64 rows .. 5 = 768 rows) by ',', an
    // optional ':cap' after a tier, e.g. "4:192,2,0|3,1" (the default with two streams).
    struct PlanItem { int tier, stream; int64_t cap; };
    PlanItem plan[12];
    int n_plan = 0;
    {
        static const char* env = getenv("LCFE_GP_PLAN");
        bool seen[6] = {false, false, false, false, false, false};
        if (env && ngs > 1) {
            int st = 0;
            for (const char* c = env; *c && n_plan < 12;) {
                if (*c == '|') { ++st; ++c; continue; }
                if (*c == ',') { ++c; continue; }
                if (*c < '0' || *c > '5') return fail_msg("lcfe_extract_device: malformed LCFE_GP_PLAN");
                PlanItem it{*c - '0', (st < ngs) ? st : ngs - 1, 0};
                ++c;
                if (*c == ':') { it.cap = atoi(c + 1); ++c; while (*c >= '0' && *c <= '9') ++c; }
                if (it.tier <= last && !seen[it.tier]) { seen[it.tier] = true; plan[n_plan++] = it; }
            }
        }
        for (int ti = last, pos = 0; ti >= 0; --ti, ++pos) {
            if (env && ngs > 1) { if (!seen[ti]) plan[n_plan++] = PlanItem{ti, 0, 0}; continue; }
            plan[n_plan++] = PlanItem{ti, pos % ngs, (ti == 4 && stream2 != stream) ? 192 : 0};
        }
    }
    for (int pi = 0; pi < n_plan; ++pi) {
        const int ti = plan[pi].tier;
        const int64_t cap = plan[pi].cap;
        const int nan_from = nan_from_of(ti, last);
        hipStream_t q = gs[plan[pi].stream];
        int rc = 0;
        switch (ti) {
#define X(id, NP, GK, ...) case id: rc = gp_tier<NP, GK>(ti, nan_from, q, kslab[id], cap); break;
            LCFE_GP_TIERS(X)
#undef X
        }
        if (rc) return rc;
        ++*n_launch;
        // light curves beyond the last tier's cap (bin 6; NaN rows and status -100 from the launch above until this one has run)
        if (ti == last && last == kGpNumTiers - 1 && long_slabs) {
            hipLaunchKernelGGL(gp_long_kernel, dim3(kGpLongGrid), dim3(kGpLongThreads), 0, q, B, bins, kGpNumTiers, O, long_slabs,
                               tickets + SET_GP2D * 8 + 7);
            HIP_TRY(hipGetLastError());
            ++*n_launch;
        }
    }
    return 0;
}

// The fit of band j (0..3 = g, r, i, z) on policy P: R holds the band's valid rows of the slice (t, f, e) in time order
// (gp1d_rows.hpp); the working set S and the NP-row matrix K (lds_double* or global_double*) are the caller's.  The band's
// four values go to orow[4 j ..), its status word to st[j].
// What the kernels of the per-band GP do for light curve i besides the set's row: nothing (the gp1d set) ...
struct Gp1dSetOnly {
    static constexpr bool kOn = false;
    static constexpr int kNcol = GP1D_NCOL;
    template <class KP> __device__ __forceinline__ Gp1dNoTail tail(int64_t, int, KP) const { return {}; }
};
// ... or the posterior at the caller's times (lcfe_gp1d_points_device; DESIGN section 9, "Per-band GP posterior"): light
// curve i has the queries q_off[i] .. q_off[i + 1] of q_t, grouped by band in perm (gp1d_group_queries_kernel: band j's
// are perm[q_off[i] + qboff[5 i + j] ..)), and of mean and sd; theta_in / theta_out [n_obj][4][3], norm [n_obj][4][4].
// The row is the 16 per-band columns.
struct Gp1dPointsOut {
    static constexpr bool kOn = true;
    static constexpr int kNcol = 4 * GP1D_NBAND;
    const int64_t* q_off;
    const double* q_t;
    const int *perm, *qboff;
    const double* theta_in;            // nullptr: fit mode
    double *mean, *sd, *theta_out, *norm;
    template <class KP>
    __device__ __forceinline__ Gp1dPointsTail<KP> tail(int64_t i, int j, KP K) const {
        const int64_t q0 = uniform_i64(q_off[i]), ib = i * GP1D_NBAND + j;
        const int g0 = uniform_int(qboff[5 * i + j]), g1 = uniform_int(qboff[5 * i + j + 1]);
        return {theta_in != nullptr, K, theta_in ? theta_in + ib * GP1D_NTHETA : nullptr, theta_out + ib * GP1D_NTHETA, norm + ib * GP1D_NNORM,
                q_t + q0, perm + q0 + g0, g1 - g0, mean + q0, sd + q0};
    }
};

template <class P, int NP, class Rows, class KP, bool IN_LDS, class PO>
__device__ __forceinline__ void gp1d_fit_band(const Rows& R, int j, const double* t, const double* f, const double* e,
                                              Gp1dLds<NP, P::NWAVES, IN_LDS>& S, KP K, double* orow, int32_t* st, const PO& po, int64_t i) {
    const int b0 = R.boff[j], m = R.boff[j + 1] - b0;
    gp1d_band<P, NP>([&](int r, double& tt, double& ff, double& ee) { const int k = R.rows[b0 + r]; tt = t[k]; ff = f[k]; ee = e[k]; }, m, S,
                     [&](const double* x, int nn, double& fv, double* gv) { gp1d_eval<P, NP, KP>(x, nn, S, K, fv, gv); },
                     orow + 4 * j, st ? st + j : nullptr, po.tail(i, j, K));
}

// MW = waves per SIMD the register allocation leaves room for (= workgroups per CU at 256 threads)
// (the loop of gp1d_kernel and gp1d_points_kernel; PO: Gp1dSetOnly, Gp1dPointsOut)
template <int NP, int ROWCAP, int T, int WNP, class PO>
__device__ __forceinline__ void gp1d_objects(const BatchView& B, const Bins& bins, int bin, int nan_from, const SetOut& O,
                                             unsigned long long* ticket, double* kslab, const PO& po) {
    using W = BlockDev<T>;
    constexpr bool kWavePath = (T == 256);
    __shared__ __attribute__((aligned(16))) unsigned char raw[gp1d_lds_bytes<NP, T, WNP>()];
    auto& LB = *reinterpret_cast<Gp1dBlockLds<NP, W::NWAVES>*>(raw);
    __shared__ Gp1dRows<T, ROWCAP, ROWCAP> R;
    __shared__ double orow[GP1D_NCOL + 3];
    __shared__ long long next_ticket;
    const int count = bins.count(gp_list(bin));
    const int* list = bins.list(gp_list(bin));
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= count) break;
        const ListObject o = take_object(B, list, pos);
        const int64_t i = o.i, s = o.s;
        const double* t = B.t + s;
        const double* f = B.f + s;
        const double* e = B.e + s;
        int32_t* st = O.st(i);
        R.build(t, f, e, B.b + s, (int)o.n);
        auto nvalid = [&](int j) { return R.boff[j + 1] - R.boff[j]; };
        bool fitted[4];
        int most = 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) { fitted[j] = R.nall[j] >= 5; most = (nvalid(j) > most) ? nvalid(j) : most; }
        // phase 1: every band that fits a WNP-row matrix, one per wavefront, side by side
        if constexpr (kWavePath) {
            const int j = threadIdx.x >> 6;
            if (nvalid(j) + 1 <= WNP) {
                auto& LW = reinterpret_cast<Gp1dWaveLds<WNP>*>(raw)[j];
                gp1d_fit_band<WaveOfBlock, WNP>(R, j, t, f, e, LW.S, (lds_double*)LW.K, orow, st, po, i);
            }
            __syncthreads();
        }
        // phase 2: the longer bands one after the other on the whole workgroup (same LDS buffer, NP-row matrix)
        if (!kWavePath || most + 1 > WNP) {
            for (int j = 0; j < 4; ++j) {
                if (kWavePath && nvalid(j) + 1 <= WNP) continue;
                gp1d_fit_band<W, NP>(R, j, t, f, e, LB.S, (lds_double*)LB.K, orow, st, po, i);
                __syncthreads();
            }
        }
        // phase 3 (tier of 160..767 rows only): a band with more valid points than the LDS matrix takes has its Gram matrix
        // in this workgroup's slab of global scratch; the working set of a kGp1dLongNP-row fit aliases the LDS buffer
        if constexpr (ROWCAP > NP) {
            if (kslab != nullptr && most + 1 > NP) {
                static_assert(sizeof(Gp1dLds<kGp1dLongNP, W::NWAVES>) <= sizeof(raw), "long-band working set must fit the LDS buffer");
                auto& LG = *reinterpret_cast<Gp1dLds<kGp1dLongNP, W::NWAVES>*>(raw);
                double* Kg = kslab + (size_t)blockIdx.x * (size_t)gp_store_doubles(kGp1dLongNP);
                for (int j = 0; j < 4; ++j) {
                    if (nvalid(j) + 1 <= NP) continue;
                    gp1d_fit_band<W, kGp1dLongNP>(R, j, t, f, e, LG, (global_double*)Kg, orow, st, po, i);
                    __syncthreads();
                }
            }
        }
        __syncthreads();
        if constexpr (!PO::kOn) {
            if (threadIdx.x == 0) gp1d_cross_band(orow, fitted);
        }
        __syncthreads();
        store_row<W>(orow, O.row(i), PO::kNcol);
        __syncthreads();
    }
    nan_fill_bins<W>(bins, 1, nan_from, O, PO::kNcol, GP1D_NSTATUS);
}

template <int NP, int ROWCAP, int T, int WNP, int MW>
__global__ __launch_bounds__(T, MW) void gp1d_kernel(BatchView B, Bins bins, int bin, int nan_from, SetOut O,
                                                   unsigned long long* ticket, double* kslab) {
    gp1d_objects<NP, ROWCAP, T, WNP>(B, bins, bin, nan_from, O, ticket, kslab, Gp1dSetOnly{});
}

// the same loop with the posterior stage as every band fit's tail (one instantiation per row of the tier table, as the set)
template <int NP, int ROWCAP, int T, int WNP, int MW>
__global__ __launch_bounds__(T, MW) void gp1d_points_kernel(BatchView B, Bins bins, int bin, int nan_from, SetOut O,
                                                          unsigned long long* ticket, double* kslab, Gp1dPointsOut po) {
    gp1d_objects<NP, ROWCAP, T, WNP>(B, bins, bin, nan_from, O, ticket, kslab, po);
}

// (kslab: one slab of global scratch per workgroup)
template <int NP, int ROWCAP, int T, int WNP, int MW>
int SetLaunch::gp1d_tier(int ti, int nan_from, double* kslab) const {
    return launch_grid(gp1d_kernel<NP, ROWCAP, T, WNP, MW>, T, {0, kslab ? kGp1dLongGrid : 0}, B.n_obj, 1, stream, dev, B, bins, ti, nan_from, O,
                       tickets + SET_GP1D * 8 + ti, kslab);
}

// ---- the long-object tier of the per-band GP (gp1d_tiers.hpp)
// slabs: kGp1dLongTierGrid Gram matrices, then kGp1dLongTierGrid working sets.  Light curves of more than kLongCap rows keep
// the NaN row and status -100 the tier-5 launch wrote.
template <class PO>
__device__ __forceinline__ void gp1d_long_objects(const BatchView& B, const Bins& bins, const SetOut& O, char* slabs, unsigned long long* ticket,
                                                  const PO& po) {
    constexpr int T = kGp1dThreads, NP = kGp1dLongTierNP;
    using W = BlockDev<T>;
    // valid rows of g, r, i, z, partitioned by band, each part in time order; the rank sort takes the bands the fit takes
    __shared__ Gp1dRows<T, kLongCap, NP - 1> R;
    __shared__ double orow[GP1D_NCOL + 3];
    __shared__ long long next_ticket;
    double* Kg = reinterpret_cast<double*>(slabs) + (size_t)blockIdx.x * (size_t)gp_store_doubles(NP);
    Gp1dLongTierWs& S = *reinterpret_cast<Gp1dLongTierWs*>(slabs + (size_t)kGp1dLongTierGrid * gp_store_doubles(NP) * 8 +
                                                         (size_t)blockIdx.x * kGp1dLongTierSBytes);
    const int count = bins.count(kGpLongList);
    const int* list = bins.list(kGpLongList);
    for (;;) {
        const int64_t pos = block_ticket(ticket, next_ticket);
        if (pos >= count) break;
        const ListObject o = take_object(B, list, pos);
        const int64_t i = o.i, s = o.s;
        if (o.n <= kLongCap) {
            const double* t = B.t + s;
            const double* f = B.f + s;
            const double* e = B.e + s;
            int32_t* st = O.st(i);
            R.build(t, f, e, B.b + s, (int)o.n);
            bool fitted[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) fitted[j] = R.nall[j] >= 5;
            for (int j = 0; j < 4; ++j) {
                gp1d_fit_band<W, NP>(R, j, t, f, e, S, (global_double*)Kg, orow, st, po, i);
                __syncthreads();
            }
            if constexpr (!PO::kOn) {
                if (threadIdx.x == 0) gp1d_cross_band(orow, fitted);
            }
            __syncthreads();
            store_row<W>(orow, O.row(i), PO::kNcol);
        }
        __syncthreads();
    }
}

__global__ __launch_bounds__(kGp1dThreads, 1) void gp1d_long_kernel(BatchView B, Bins bins, SetOut O, char* slabs, unsigned long long* ticket) {
    gp1d_long_objects(B, bins, O, slabs, ticket, Gp1dSetOnly{});
}

__global__ __launch_bounds__(kGp1dThreads, 1) void gp1d_points_long_kernel(BatchView B, Bins bins, SetOut O, char* slabs, unsigned long long* ticket,
                                                                         Gp1dPointsOut po) {
    gp1d_long_objects(B, bins, O, slabs, ticket, po);
}

// The queries of every light curve grouped by band (1..4 = g, r, i, z; any other code joins no group and stays NaN): a
// stable counting pass, one wavefront per light curve.  perm[q_off[i] + k]: the k-th query of the grouped order as an index
// into the light curve's list; qboff[5 i + j]: where band j's group starts.
constexpr int kGp1dGroupWaves = 4;
__global__ __launch_bounds__(64 * kGp1dGroupWaves) void gp1d_group_queries_kernel(const int64_t* q_off, const uint8_t* q_band, int64_t n_obj, int* perm,
                                                                          int* qboff) {
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * kGp1dGroupWaves;
    for (int64_t o = (int64_t)blockIdx.x * kGp1dGroupWaves + (threadIdx.x >> 6); o < n_obj; o += stride) {
        const int64_t q0 = uniform_i64(q_off[o]);
        const int nq = (int)(uniform_i64(q_off[o + 1]) - q0);
        const uint8_t* qb = q_band + q0;
        int cnt[GP1D_NBAND] = {0, 0, 0, 0}, off[GP1D_NBAND];
        for (int k = lane; k < nq; k += 64) {
            const int b = qb[k];
#pragma unroll
            for (int j = 0; j < GP1D_NBAND; ++j) cnt[j] += (b == j + 1) ? 1 : 0;
        }
        int run = 0;
#pragma unroll
        for (int j = 0; j < GP1D_NBAND; ++j) { off[j] = run; run += WaveDev::sum(cnt[j]); }
        if (lane == 0) {
#pragma unroll
            for (int j = 0; j < GP1D_NBAND; ++j) qboff[5 * o + j] = off[j];
            qboff[5 * o + GP1D_NBAND] = run;
        }
        for (int base = 0; base < nq; base += 64) {
            const int k = base + lane;
            const int b = (k < nq) ? (int)qb[k] : 0;
#pragma unroll
            for (int j = 0; j < GP1D_NBAND; ++j) {
                const unsigned long long mk = __ballot(b == j + 1);
                if (b == j + 1) perm[q0 + off[j] + WaveDev::prefix(mk)] = k;
                off[j] += popcll(mk);
            }
        }
    }
}

// NaN in the n doubles at p (the outputs of lcfe_gp1d_points_device before a band writes its own)
__global__ __launch_bounds__(256) void gp1d_points_nan_kernel(double* p, int64_t n) {
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n; k += (int64_t)gridDim.x * 256) p[k] = qnan();
}

// The GP bins are reused (by rows of the whole object): bins 0..2 run with a Gram matrix as large as the
// object; bins 3..5 (160..767 rows) with the 160-row matrix, a band of 160..767 valid points with the 768-row one in
// global scratch; bin 6 (more than 767 rows) in the long-object tier when the workspace holds its slabs (long_slab),
// NaN and status -100 otherwise.
int SetLaunch::launch_gp1d(double* kslab) const {
    const int last = gp_last_tier(max_len);
    for (int ti = last; ti >= 0; --ti) {
        const int nan_from = nan_from_of(ti, last);
        int rc = 0;
        // the table of gp1d_tiers.hpp; tiers 3..5 share its last row, the only one with a global-scratch matrix
        switch ((ti < kGp1dKernelTiers) ? ti : kGp1dKernelTiers - 1) {
#define X(id, NP, ROWCAP, WNP, MW) \
            case id: rc = gp1d_tier<NP, ROWCAP, kGp1dThreads, WNP, MW>(ti, nan_from, (ROWCAP > NP) ? kslab : nullptr); break;
            LCFE_GP1D_KERNEL_TIERS(X)
#undef X
        }
        if (rc) return rc;
        ++*n_launch;
    }
    // light curves of more than 767 rows (bin 6): they overwrite the NaN rows and status -100 of the tier-5 launch, which
    // ran before them on this stream.  Last on the stream, so that the short tiers do not wait for 8 workgroups that may
    // take seconds per light curve.
    if (long_slabs && max_len > SetTraits<SET_GP1D>::long_above) {
        hipLaunchKernelGGL(gp1d_long_kernel, dim3(kGp1dLongTierGrid), dim3(kGp1dThreads), 0, stream, B, bins, O, long_slabs,
                           tickets + SET_GP1D * 8 + 7);
        HIP_TRY(hipGetLastError());
        ++*n_launch;
    }
    return 0;
}

template <int SET, int CAP>
int SetLaunch::tier(int bin, int nan_from, hipStream_t q, unsigned long long* tk, int64_t cap) const {
    constexpr int chunk = SetTraits<SET>::chunk;
    return launch_grid(set_kernel<SET, CAP>, 64, {0, cap}, B.n_obj, chunk, q, dev, B, bins, bin, nan_from, O, tk, chunk);
}

template <int SET>
int SetLaunch::launch_set() const {
    using T = SetTraits<SET>;
    const int last = last_tier(max_len, T::max_tier);
    for (int ti = 0; ti <= last; ++ti) {
        const int rc = for_tier(ti, [&](auto cap) -> int {
            if constexpr (cap() <= kTiers[T::max_tier])      // (no 2048-row kernel for a set whose tiers end at 1024 rows)
                return this->template tier<SET, cap()>(ti, nan_from_of(ti, last), stream, tickets + T::ticket_base + ti);
            return 0;
        });
        if (rc) return rc;
        ++*n_launch;
    }
    // the long-object tier: bin 6 (more than 2048 rows), bin 4 too where the set's LDS tiers end at 1024 rows, and the set's
    // overflow list (research: more than 4096 days of r band)
    if (long_slabs && (max_len > T::long_above || T::overflow_list >= 0)) {
        const int rc = long_tier<SET>(6, (T::max_tier < 4) ? 4 : -1, T::overflow_list);
        if (rc) return rc;
        ++*n_launch;
    }
    return 0;
}

// LCFE_FIT_NARROW=0 queues the bands of up to 16 rows on the 32-row fit lists, as before the 16-row tier (A/B measurements)
static bool fit_narrow_enabled() {
    static const bool on = [] { const char* e = getenv("LCFE_FIT_NARROW"); return !(e && e[0] == '0'); }();
    return on;
}

// tuning knob: LCFE_FIT_WAVES_<rows>=k caps the fit kernels of that band-length tier at k wavefronts per CU (their LDS
// regions otherwise take most of a CU and keep the LDS-resident GP tiers off it); 0: no cap
static int fit_waves_cap(int bcap) {
    char name[40];
    snprintf(name, sizeof name, "LCFE_FIT_WAVES_%d", bcap);
    const char* e = getenv(name);
    return (e && atoi(e) > 0) ? atoi(e) : 0;
}

// one fit kernel over list `tier` of the lists whose ticket counters start at tickets[ticket_base]; one ticket = 8 fits.
// (The kernel of the narrow tier's host drains the narrow list as well and gets that list's counter too.)
template <class K, class Ws>
int SetLaunch::fit_stream(K kernel, int tier, int fits_per_object, int ticket_base, const Ws& F) const {
    unsigned long long* tk = tickets + ticket_base;
    const int rc = launch_grid(kernel, 64, {fit_waves_cap(fit_tier_cap(tier)), 0}, fits_per_object * B.n_obj, 8, stream, dev, B, bins, F, tier, O,
                               tk + tier, tk + kFitNarrowTier);
    if (!rc) ++*n_launch;
    return rc;
}

// The two fit-by-fit families as launch_fits takes them: the set, its share of the workspace, the partition kernel, the
// fit kernels of one band-length tier, the lists of the light curves the fit tiers do not take, and what follows the fits.
struct BazinFits {
    using Ws = FitWs;
    static constexpr int kSet = SET_BAZIN, kFallbackList = kBazinFallbackList, kLongList = kBazinLongList;
    template <int CAP> static constexpr auto partition = bazin_partition_kernel<CAP>;
    template <int T> static int fits(const SetLaunch& L, const Ws& F) {
        return L.fit_stream(bazin_fit_kernel<fit_tier_cap(T)>, T, kBazinFits, kFitTicketBase, F);
    }
    // the cross-band columns, once all fits are in
    static int epilogue(const SetLaunch& L) {
        hipLaunchKernelGGL(bazin_cross_kernel, dim3((unsigned)((L.B.n_obj + 255) / 256)), dim3(256), 0, L.stream, L.B, L.O);
        HIP_TRY(hipGetLastError());
        ++*L.n_launch;
        return 0;
    }
};
struct DeclineFits {
    using Ws = PlWs;
    static constexpr int kSet = SET_POWERLAW, kFallbackList = kPowerlawFallbackList, kLongList = kPowerlawLongList;
    template <int CAP> static constexpr auto partition = powerlaw_partition_kernel<CAP>;
    // the two-parameter fits (list A), then the three-parameter ones (list B)
    template <int T> static int fits(const SetLaunch& L, const Ws& F) {
        if (const int rc = L.fit_stream(powerlaw_fit_kernel<2, fit_tier_cap(T)>, T, kPlFitsA, kPlTicketA, F)) return rc;
        return L.fit_stream(powerlaw_fit_kernel<3, fit_tier_cap(T)>, T, kPlFitsB, kPlTicketB, F);
    }
    static int epilogue(const SetLaunch&) { return 0; }
};

// A fit-by-fit family: the partition pass per object tier, the object-level kernel for the light curves with a band beyond
// the largest fit tier, the fit kernels per band-length tier (longest first), the family's epilogue, the long-object tier.
template <class Fam>
int SetLaunch::launch_fits(const typename Fam::Ws& F) const {
    const int last = last_tier(max_len, 4);
    unsigned long long* tk = tickets + Fam::kSet * 8;
    for (int ti = 0; ti <= last; ++ti) {
        const int rc = for_tier(ti, [&](auto cap) {
            return launch_grid(Fam::template partition<cap()>, 64, {}, B.n_obj, 8, stream, dev, B, bins, ti, nan_from_of(ti, last), F, O, tk + ti,
                               8, fit_narrow_enabled() ? 1 : 0);
        });
        if (rc) return rc;
        ++*n_launch;
    }
    // light curves with a band of more rows than the largest fit tier: the object-level kernel (all columns).  A small grid,
    // and AHEAD of the fit tiers: the list is normally empty, but every workgroup of this kernel needs 136 KiB of LDS -- at the
    // end of the stream it sat in the dispatcher for 100-180 ms, until a GP tier released a whole CU (tools/step_timeline.py)
    int rc = tier<Fam::kSet, kFitObjectRows>(Fam::kFallbackList, kNumBins, stream, tk + 5, 32);
    if (rc) return rc;
    ++*n_launch;
    // the tiers of fit_tier_table.hpp that have kernels of their own, longest first
    for (int t = kFitTiers - 1; t >= 0 && !rc; --t)
        switch (t) {
#define X(id, BCAP, LANES, GROUPS, WB, WD, KERNEL) case id: if constexpr (KERNEL) rc = Fam::template fits<id>(*this, F); break;
            LCFE_FIT_TIERS(X)
#undef X
        }
    if (!rc) rc = Fam::epilogue(*this);
    if (rc) return rc;
    // the long-object tier: more rows than the LDS tiers take (bin 6), or than the object-level kernel takes with a band
    // beyond the fit tiers (all columns)
    if (long_slabs && max_len > SetTraits<Fam::kSet>::long_above) {
        rc = long_tier<Fam::kSet>(6, Fam::kLongList, -1);
        if (rc) return rc;
        ++*n_launch;
    }
    return 0;
}

// (cap: for a list expected to be short: every wavefront's first ticket is an atomic on one counter)
template <int CAP>
int SetLaunch::stat_lean(int bin, hipStream_t q, unsigned long long* tk, int64_t cap) const {
    return launch_grid(stat_lean_kernel<CAP>, 64, {0, cap}, B.n_obj, 8, q, dev, B, bins, bin, O, tk, 8);
}

int launch_stat_plan(const BatchView& B, const Bins& bins, hipStream_t stream) {
    const int64_t grid = (B.n_obj + kPlanThreads / 8 - 1) / (kPlanThreads / 8) + 3;
    hipLaunchKernelGGL(stat_plan_kernel, dim3((unsigned)grid), dim3(kPlanThreads), 0, stream, B, bins);
    HIP_TRY(hipGetLastError());
    return 0;
}

int launch_stat_lanes_all(const BatchView& B, const Bins& bins, int retry, const SetOut& O, hipStream_t stream) {
    const int64_t grid = (B.n_obj + 3) / 4 + 6;
    hipLaunchKernelGGL(stat_lanes_all_kernel, dim3((unsigned)grid), dim3(64), 0, stream, B, bins, retry, O);
    HIP_TRY(hipGetLastError());
    return 0;
}

// LCFE_STAT_LANES=0 keeps the one-light-curve-per-wavefront kernels for the 128- and 256-row tiers (A/B measurements)
static bool stat_lanes_enabled() {
    const char* e = getenv("LCFE_STAT_LANES");
    return !(e && e[0] == '0');
}

// Statistics: lean kernels for the tiers up to 512 rows, the general kernel for the longer tiers,
// for the lean kernels' fallback list and for the NaN rows of over-long objects.
int SetLaunch::launch_stat(hipStream_t s1, hipStream_t s2) const {
    SetLaunch G = *this;                // the general kernel's launches: the set has no status words
    G.O = O.without_status();
    const int last = last_tier(max_len, 4);
    unsigned long long* tk = tickets + SET_STAT * 8;
    // The tier kernels are independent (disjoint objects): with side streams they are enqueued side by side, so the
    // ramp-down of one tier is filled by the waves of the others; they are joined before the fallback launch.
    //   s2:     the tiers of more than 256 rows, from the start
    //   stream: the plan kernels (which lanes kernel takes a light curve of up to 256 rows), then the lanes kernels
    //   s1:     after the plan kernels, the 256-row tier's one-light-curve-per-wavefront kernel
    const bool lanes = stat_lanes_enabled();
    const bool fork = (s1 != stream) && (s2 != stream) && last >= 1;
    hipStream_t q_long = fork ? s2 : stream, q_mid = fork ? s1 : stream;
    if (fork && stream_wait(s2, stream)) return 1;
    for (int ti = 2; ti <= last; ++ti) {
        int rc = 0;
        if (ti == 2) {
            if (!lanes) rc = stat_lean<512>(ti, q_long, tk + ti);   // (else: after its plan kernel)
        } else {
            rc = for_tier(ti, [&](auto cap) -> int {
                if constexpr (cap() > 512) return G.tier<SET_STAT, cap()>(ti, nan_from_of(ti, last), q_long, tk + ti);
                return 0;
            });
        }
        if (rc) return rc;
        ++*n_launch;
    }
    if (lanes) {
        // one routing pass over the tiers of up to 512 rows (stat_plan_kernel): lanes lists + the retry list
        const int rc = launch_stat_plan(B, bins, stream);
        if (rc) return rc;
        ++*n_launch;
    }
    if (fork) {
        const hipStream_t after_plan[2] = {s1, s2};
        if (stream_wait(after_plan, (lanes && last >= 2) ? 2 : 1, stream)) return 1;
    }
    {
        int rc = 0;
        if (lanes) {
            // what the lanes variants do not take: one light curve per wavefront, sized for the longest tier present;
            // a light curve whose rows turn out not to ascend in time goes to the general kernel's list
            if (last >= 2) rc = stat_lean<512>(kStatRetryList, q_long, tk + 2);
            else if (last == 1) rc = stat_lean<256>(kStatRetryList, q_mid, tk + 1, 512);
            if (!rc) rc = launch_stat_lanes_all(B, bins, kStatFallbackList, O, stream);
            if (!rc && last < 1) rc = stat_lean<128>(kStatRetryList, stream, tk + 6, 512);
            *n_launch += 2;
        } else {
            if (last >= 1) rc = stat_lean<256>(1, q_mid, tk + 1);
            if (!rc) rc = stat_lean<128>(0, stream, tk + 0);
            *n_launch += 2;
        }
        if (rc) return rc;
    }
    if (fork && (stream_wait(stream, s1) || stream_wait(stream, s2))) return 1;
    // fallback list of the lean tiers (+ the NaN rows when no general tier ran): normally empty or a
    // handful of objects, so a quarter-chip grid keeps the launch short
    const int nan_from = (last <= 2) ? last + 1 : kNumBins;
    const int64_t fb_grid = 256;
    int rc = for_tier((last < 2) ? last : 2, [&](auto cap) -> int {
        if constexpr (cap() <= 512) return G.tier<SET_STAT, cap()>(kStatFallbackList, nan_from, stream, tk + 5, fb_grid);
        return 0;
    });
    if (rc) return rc;
    ++*n_launch;
    if (long_slabs && max_len > SetTraits<SET_STAT>::long_above) {
        rc = G.long_tier<SET_STAT>(6, -1, -1);
        if (rc) return rc;
        ++*n_launch;
    }
    return 0;
}

#include "colnames.inc"

bool set_implemented(int set) { return set_known(set); }
// the table's column counts are those of the generated column names (the hole at bit 13 has none)
static_assert(sizeof kColCount / sizeof kColCount[0] == NUM_ALL_SETS && kColCount[SET_UNASSIGNED] == 0, "colnames.inc: one table per mask bit");
#define LCFE_CHECK_COLS(ID, ...) static_assert(SetTraits<ID>::ncols == kColCount[ID], "feature_sets.hpp and colnames.inc disagree on the columns of " #ID);
LCFE_SET_TABLE(LCFE_CHECK_COLS)
#undef LCFE_CHECK_COLS

// profile of every set of the last call this thread made with prof != NULL (lcfe_last_set_profile; lcfe_last_ext_profile
// reads the extension sets' entries)
thread_local double g_set_ms[NUM_ALL_SETS];
thread_local int32_t g_set_launches[NUM_ALL_SETS];
// the numbered sets and the extension sets are exactly the public tables; everything above them is a registered set
static_assert(NUM_SETS == LCFE_NUM_SETS && SET_ADVANCED == LCFE_XSET_ADVANCED && SET_ADVANCED + 1 == LCFE_NUM_SETS + LCFE_NUM_XSETS,
              "set ids of feature_sets.hpp and include/lcfe.h");
static_assert(SET_CESIUM == LCFE_RSET_CESIUM && SET_FOURIER == LCFE_RSET_FOURIER && SET_UNASSIGNED == LCFE_NUM_SETS + LCFE_NUM_XSETS,
              "registered set ids of feature_sets.hpp and include/lcfe.h; the bit after the extension sets stays unassigned");

// Non-blocking side streams per device, created on first use and kept for the life of the process.
constexpr int kSideStreams = 5;       // [0] Bazin, [1] decline fits, [2] streaming sets + GP tiers, [3], [4] further GP tiers
hipStream_t g_side[16][kSideStreams];
bool g_side_ready[16] = {false};
std::mutex g_side_mutex;
int side_streams(int dev, hipStream_t* out) {
    if (dev < 0 || dev >= 16) return 1;
    std::lock_guard<std::mutex> lock(g_side_mutex);
    if (!g_side_ready[dev]) {
        for (int k = 0; k < kSideStreams; ++k)
            if (hipStreamCreateWithFlags(&g_side[dev][k], hipStreamNonBlocking) != hipSuccess) return 1;
        g_side_ready[dev] = true;
    }
    for (int k = 0; k < kSideStreams; ++k) out[k] = g_side[dev][k];
    return 0;
}

// staging buffers + events of the host-buffer entry point, per device
struct HostPathPool {
    static constexpr int NBUF = 9;     // offsets, t, flux, err, band, z, out, status, workspace
    void* buf[NBUF] = {};
    size_t cap[NBUF] = {};
    hipEvent_t ev[4] = {};
    std::mutex mutex;
};
HostPathPool g_pool[16];

// what workspace.hpp takes from the kernels' own structures; every size a multiple of the regions' 256-byte rounding
// (the 2-D GP tiers' slabs: gp_tier_slab_bytes of gp_tier_table.hpp, which holds them to the same rounding)
static_assert(kGp1dLongBytes % 256 == 0 && GpLongTier::kBytes % 256 == 0 && kGp1dLongTierBytes % 256 == 0, "slab sizes");
const WsSizes kWsSizes = [] {
    WsSizes z{{}, kGp1dLongBytes, {}};
    for (int ti = 0; ti < kGpNumTiers; ++ti) z.gp_slab[ti] = gp_tier_slab_bytes(ti);
    for (int s = 0; s < NUM_ALL_SETS; ++s)
        z.long_slab[s] = for_set(s, [](auto tag) -> size_t {
            if constexpr (tag() == SET_GP2D) return GpLongTier::kBytes;
            else if constexpr (tag() == SET_GP1D) return kGp1dLongTierBytes;
            else return kLongGrid * long_slab_bytes<tag()>();
        });
    return z;
}();

FitWs bazin_ws(const WsLayout& L, void* ws) {
    double* rows = (double*)L.at(ws, WS_BAZIN_ROWS);
    return FitWs{rows, rows + L.np, rows + 2 * L.np, (int*)L.at(ws, WS_BAZIN_PBOFF), (int*)L.at(ws, WS_BAZIN_FITS), kBazinFits * (int64_t)L.no};
}
PlWs powerlaw_ws(const WsLayout& L, void* ws) {
    double *rows = (double*)L.at(ws, WS_PL_ROWS), *peak = (double*)L.at(ws, WS_PL_PEAK);
    return PlWs{rows, rows + L.np, peak, peak + kPlBands * L.no, (int*)L.at(ws, WS_PL_PBOFF), (int*)L.at(ws, WS_PL_KK),
                (int*)L.at(ws, WS_PL_FITS_A), (int*)L.at(ws, WS_PL_FITS_B), kPlFitsA * (int64_t)L.no, kPlFitsB * (int64_t)L.no};
}

// ---- augmentation (augment.hpp): count, prefix sum in place, write.  One wavefront per INPUT object -- its first epoch is
// found once for the k copies -- and kAugWaves objects per workgroup; the grids stride over the objects.
constexpr int kAugWaves = 4;
constexpr int kAugScanThreads = 256, kAugScanItems = 8, kAugScanTile = kAugScanThreads * kAugScanItems;
// workspace: [0, 256) the bad-plan flag, then the first epochs double[n_obj], then one partial sum per scan tile
constexpr size_t kAugWsHeader = 256;
struct AugWs {
    int* flag;
    double* tmin;
    int64_t* tile_sum;
    int64_t tiles;
    size_t bytes;
    AugWs(void* ws, int64_t n_obj, int k) {
        tiles = (n_obj * k + kAugScanTile - 1) / kAugScanTile;
        const size_t tmin_bytes = ((size_t)n_obj * 8 + 255) & ~(size_t)255;
        flag = (int*)ws;
        tmin = (double*)((char*)ws + kAugWsHeader);
        tile_sum = (int64_t*)((char*)ws + kAugWsHeader + tmin_bytes);
        bytes = kAugWsHeader + tmin_bytes + (((size_t)tiles * 8 + 255) & ~(size_t)255);
    }
};

__global__ __launch_bounds__(64 * kAugWaves) void augment_count_kernel(AugIn A, AugPlan P, int64_t n_obj, double* tmin, int64_t* offsets_out,
                                                                        int* flag) {
    if (blockIdx.x == 0 && threadIdx.x == 0) offsets_out[0] = 0;
    const int64_t stride = (int64_t)gridDim.x * kAugWaves;
    for (int64_t i = (int64_t)blockIdx.x * kAugWaves + (threadIdx.x >> 6); i < n_obj; i += stride)
        if (!aug_count_object<AugWave>(A, P, i, tmin, offsets_out + 1) && AugWave::lane() == 0) atomicOr(flag, 1);
}

// sum of the workgroup's values v (one per thread) below each thread, and their total: Hillis-Steele over LDS
__device__ __forceinline__ int64_t aug_block_exclusive(int64_t v, int64_t* total) {
    __shared__ int64_t buf[2][kAugScanThreads];
    const int tid = threadIdx.x;
    int cur = 0;
    buf[0][tid] = v;
    __syncthreads();
    for (int d = 1; d < kAugScanThreads; d <<= 1) {
        buf[cur ^ 1][tid] = buf[cur][tid] + ((tid >= d) ? buf[cur][tid - d] : 0);
        cur ^= 1;
        __syncthreads();
    }
    const int64_t incl = buf[cur][tid];
    *total = buf[cur][kAugScanThreads - 1];
    __syncthreads();
    return incl - v;
}

// x[0..m) in tiles of kAugScanTile entries: the sum of every tile ...
__global__ __launch_bounds__(kAugScanThreads) void augment_scan_tiles_kernel(const int64_t* x, int64_t m, int64_t* tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * kAugScanTile + (int64_t)threadIdx.x * kAugScanItems;
    int64_t s = 0;
#pragma unroll
    for (int j = 0; j < kAugScanItems; ++j) s += (base + j < m) ? x[base + j] : 0;
    int64_t total;
    aug_block_exclusive(s, &total);
    if (threadIdx.x == 0) tile_sum[blockIdx.x] = total;
}
// ... the tile sums into the sums of the tiles before each (one workgroup), and the grand total -- -1 for a bad plan ...
__global__ __launch_bounds__(kAugScanThreads) void augment_scan_sums_kernel(int64_t* tile_sum, int64_t tiles, const int* flag, int64_t* n_points_out) {
    int64_t carry = 0;
    for (int64_t base = 0; base < tiles; base += kAugScanThreads) {
        const int64_t j = base + threadIdx.x;
        const int64_t v = (j < tiles) ? tile_sum[j] : 0;
        int64_t total;
        const int64_t ex = aug_block_exclusive(v, &total);
        if (j < tiles) tile_sum[j] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) *n_points_out = *flag ? -1 : carry;
}
// ... and every entry replaced by the sum of the entries up to and including it
__global__ __launch_bounds__(kAugScanThreads) void augment_scan_apply_kernel(int64_t* x, int64_t m, const int64_t* tile_sum) {
    const int64_t base = (int64_t)blockIdx.x * kAugScanTile + (int64_t)threadIdx.x * kAugScanItems;
    int64_t v[kAugScanItems], s = 0;
#pragma unroll
    for (int j = 0; j < kAugScanItems; ++j) { v[j] = (base + j < m) ? x[base + j] : 0; s += v[j]; }
    int64_t total;
    int64_t run = tile_sum[blockIdx.x] + aug_block_exclusive(s, &total);
#pragma unroll
    for (int j = 0; j < kAugScanItems; ++j) {
        run += v[j];
        if (base + j < m) x[base + j] = run;
    }
}

// RECIPE: the write pass with the steps of lcfe_augment_recipe_device (augment.hpp); the plain pass is compiled without them
template <bool RECIPE>
__global__ __launch_bounds__(64 * kAugWaves) void augment_write_kernel(AugIn A, AugPlan P, AugOut O, int64_t n_obj, const double* tmin,
                                                                        const int* flag) {
    __shared__ int hist[kAugWaves][64];
    if (*flag) return;                       // a bad plan: the counts are void, nothing is written
    const int64_t stride = (int64_t)gridDim.x * kAugWaves;
    for (int64_t i = (int64_t)blockIdx.x * kAugWaves + (threadIdx.x >> 6); i < n_obj; i += stride)
        aug_write_object<AugWave, RECIPE>(A, P, O, i, tmin, hist[threadIdx.x >> 6]);
}

// the plain call and the recipe call: the same checks, the same five launches; `fn` names the entry point in the messages
template <bool RECIPE>
int augment_launch(const std::string& fn, int device, void* stream_, int64_t n_obj, int64_t n_points, int k, const AugIn& A,
                          const AugPlan& P, const AugOut& O, int64_t* d_n_points_out, void* d_workspace, size_t workspace_bytes) {
    g_err.clear();
    if (k < 1) return fail_msg(fn + ": k must be at least 1");
    if (n_obj < 0 || n_points < 0) return fail_msg(fn + ": negative size");
    if (lcfe_augment_capacity(n_points, k) < 0 || n_obj > (INT64_MAX >> 4) / k) return fail_msg(fn + ": n_points * k or n_obj * k overflows");
    if (P.keep_rule < 0 || P.keep_rule >= AUG_KEEP_RULES) return fail_msg(fn + ": unknown keep_rule " + std::to_string(P.keep_rule));
    if (!A.offsets || !O.offsets || !d_n_points_out) return fail_msg(fn + ": null offsets or n_points_out");
    if (n_obj > 0 && (!P.scale || !P.stretch || !P.shift || !P.noise_scale || !P.dropout || !P.band_noise || !P.seed))
        return fail_msg(fn + ": null plan array");
    if (n_points > 0 && (!A.t || !A.f || !A.e || !A.b || !O.t || !O.f || !O.e || !O.b)) return fail_msg(fn + ": null sample array");
    const AugWs W(d_workspace, n_obj, k);
    if (!d_workspace || workspace_bytes < W.bytes) return fail_msg(fn + ": workspace smaller than lcfe_augment_workspace_bytes(n_obj, k)");
    if (W.tiles > 0x7fffffff) return fail_msg(fn + ": more than 2^42 output objects");
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(fn + ": cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStream_t stream = (hipStream_t)stream_;
    HIP_TRY(hipMemsetAsync(d_workspace, 0, kAugWsHeader, stream));
    if (n_obj == 0) {
        HIP_TRY(hipMemsetAsync(O.offsets, 0, sizeof(int64_t), stream));
        HIP_TRY(hipMemsetAsync(d_n_points_out, 0, sizeof(int64_t), stream));
        return 0;
    }
    const int64_t groups = (n_obj + kAugWaves - 1) / kAugWaves, cap = (int64_t)num_cus(dev) * 8;
    const unsigned grid = (unsigned)((groups < cap) ? groups : cap);
    const int64_t m = n_obj * k;
    hipLaunchKernelGGL(augment_count_kernel, dim3(grid), dim3(64 * kAugWaves), 0, stream, A, P, n_obj, W.tmin, O.offsets, W.flag);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(augment_scan_tiles_kernel, dim3((unsigned)W.tiles), dim3(kAugScanThreads), 0, stream, O.offsets + 1, m, W.tile_sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(augment_scan_sums_kernel, dim3(1), dim3(kAugScanThreads), 0, stream, W.tile_sum, W.tiles, W.flag, d_n_points_out);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(augment_scan_apply_kernel, dim3((unsigned)W.tiles), dim3(kAugScanThreads), 0, stream, O.offsets + 1, m, W.tile_sum);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(augment_write_kernel<RECIPE>, dim3(grid), dim3(64 * kAugWaves), 0, stream, A, P, O, n_obj, W.tmin, W.flag);
    HIP_TRY(hipGetLastError());
    return 0;
}

// ---- sequence tensors (sequence.hpp): one wavefront per object, kSeqWaves objects per workgroup; the grid strides over
// the objects.  No LDS and no workspace: an object is streamed from the batch.
constexpr int kSeqWaves = 4;

__global__ __launch_bounds__(64 * kSeqWaves) void sequences_kernel(SeqIn A, SeqOut O, int64_t n_obj, int64_t max_length, int normalize) {
    const int64_t stride = (int64_t)gridDim.x * kSeqWaves;
    for (int64_t i = (int64_t)blockIdx.x * kSeqWaves + (threadIdx.x >> 6); i < n_obj; i += stride)
        seq_object<WaveOfBlock>(A, O, i, max_length, normalize != 0);
}

// What lcfe_gp2d_grid_device and lcfe_gp2d_points_device enqueue once their arguments are checked: binning, the sort, and
// the tiers' kernels with `O` (GpGridOut, GpPointsOut) as their column source and outputs.
template <class Out>
int gp_grid_enqueue(const char* me, int device, hipStream_t q, int64_t n_obj, int64_t n_points, int64_t max_len, const BatchView& B,
                    const Out& O, void* d_workspace, size_t workspace_bytes) {
    const WsLayout L(kWsSizes, 1 << SET_GP2D, n_obj, n_points, max_len, true);
    if (!d_workspace || workspace_bytes < L.total)
        return fail_msg(std::string(me) + "workspace smaller than " + Out::kWorkspaceFn + "(n_obj, n_points, max_len)");
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(std::string(me) + "cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    unsigned long long* tickets = (unsigned long long*)d_workspace;
    const Bins bins{(int*)L.at(d_workspace, WS_LISTS), (int*)((char*)d_workspace + kWsCounts), n_obj};
    HIP_TRY(hipMemsetAsync(d_workspace, 0, kWsHeader, q));
    hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((n_obj + kBinThreads - 1) / kBinThreads)), dim3(kBinThreads), 0, q, B.offsets, n_obj,
                       bins.lists, bins.counts);
    HIP_TRY(hipGetLastError());
    const int last = gp_last_tier(max_len);
    hipLaunchKernelGGL(gp_sort_kernel, dim3((unsigned)(last + 1)), dim3(kGpSortThreads), 0, q, B.offsets, bins);
    HIP_TRY(hipGetLastError());
    // the set's tuning knob: LCFE_GP_GRID_<rows>=k caps the workgroups of a tier (SetLaunch::gp_tier; 2048: the long-object
    // tier) -- with k = 1 every light curve of the tier goes through ONE workgroup, which is how the tests reach the state a
    // workgroup carries from one light curve to the next
    auto grid_cap = [](int np, int64_t cap) -> int64_t {
        char name[40];
        snprintf(name, sizeof name, "LCFE_GP_GRID_%d", np);
        const char* e = getenv(name);
        return (e && atoi(e) > 0 && (cap < 1 || atoi(e) < cap)) ? atoi(e) : cap;
    };
    // the tiers longest first on the caller's stream; every light curve is in the list of one of them or in the long list
    for (int ti = last; ti >= 0; --ti) {
        int rc = 0;
        switch (ti) {
#define X(id, NP, GK, T, WV, FUSE, COMPACT, SLABS)                                                                                   \
    case id:                                                                                                                         \
        rc = launch_grid(gp_grid_kernel<NP, GK, Out>, T, {0, grid_cap(NP, GK ? SLABS : 0)}, n_obj, 1, q, dev, B, bins, ti, O,             \
                         (double*)L.at(d_workspace, WS_GP_TIER + id), tickets + SET_GP2D * 8 + id);                                  \
        break;
            LCFE_GP_TIERS(X)
#undef X
        }
        if (rc) return rc;
    }
    if (max_len > kGpLastCap) {
        hipLaunchKernelGGL(gp_grid_long_kernel<Out>, dim3((unsigned)grid_cap(kGpLongNP, kGpLongGrid)), dim3(kGpLongThreads), 0, q, B, bins, kGpNumTiers, O,
                           L.at(d_workspace, WS_LONG + SET_GP2D), tickets + SET_GP2D * 8 + 7);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

// ---- GP-resampled copies (gp_resample.hpp): one wavefront per source object (query) or per copy (write), kAugWaves of them
// per workgroup; the grids stride.  No LDS and no workspace.
__global__ __launch_bounds__(64 * kAugWaves) void gp_resample_query_kernel(GpResSource S, GpResCopies C, GpResPlan P, int64_t n_src, int origin,
                                                                         int64_t* q_off, double* q_t, double* q_lam) {
    const int64_t stride = (int64_t)gridDim.x * kAugWaves;
    for (int64_t o = (int64_t)blockIdx.x * kAugWaves + (threadIdx.x >> 6); o < n_src; o += stride)
        gp_res_query_object<AugWave>(S, C, P, o, n_src, origin, q_off, q_t, q_lam);
}

__global__ __launch_bounds__(64 * kAugWaves) void gp_resample_write_kernel(GpResCopies C, GpResPlan P, int64_t n_copies, const double* mean,
                                                                         const double* var, const double* n1, const double* n2,
                                                                         const int32_t* src_status, int nst, double* flux_out, double* err_out,
                                                                         int32_t* status_out) {
    const int64_t stride = (int64_t)gridDim.x * kAugWaves;
    for (int64_t oc = (int64_t)blockIdx.x * kAugWaves + (threadIdx.x >> 6); oc < n_copies; oc += stride)
        gp_res_write_copy<AugWave>(C, P, oc, mean, var, n1, n2, src_status, nst, flux_out, err_out, status_out);
}

}  // namespace

extern "C" {

#ifdef LCFE_TRF_PROF
// debug builds only: read and reset the TRF phase counters
int lcfe_debug_trf_prof(unsigned long long* out8) {
    if (hipMemcpyFromSymbol(out8, HIP_SYMBOL(lcfe::g_trf_prof), 64) != hipSuccess) return 1;
    unsigned long long z[8] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lcfe::g_trf_prof), z, 64) != hipSuccess) return 1;
    return 0;
}
#endif

#ifdef LCFE_DEBUG
// debug builds only: read and reset the counters of the bounds-checked lanes kernels
// (out4: indices outside the LDS buffer, damaged canary words, the last bad index, the length of its buffer)
int lcfe_debug_lanes_check(unsigned int* out4) {
    if (hipDeviceSynchronize() != hipSuccess) return 1;
    if (hipMemcpyFromSymbol(out4, HIP_SYMBOL(lcfe::g_lanes_check), 16) != hipSuccess) return 1;
    unsigned int z[4] = {0, 0, 0, 0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lcfe::g_lanes_check), z, 16) != hipSuccess) return 1;
    return 0;
}
#endif

#ifdef LCFE_PHASE_PROF
// debug builds only: read and reset the phase cycle counters
int lcfe_debug_phase_prof(unsigned long long* out32) {
    if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(lcfe::g_phase_prof), 256) != hipSuccess) return 1;
    unsigned long long z[32] = {0};
    if (hipMemcpyToSymbol(HIP_SYMBOL(lcfe::g_phase_prof), z, 256) != hipSuccess) return 1;
    return 0;
}
#endif

int lcfe_version(void) { return 2; }     // 2: lcfe_stats grew with LCFE_NUM_SETS = 12

int lcfe_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* lcfe_last_error(void) { return g_err.c_str(); }

int64_t lcfe_max_points(void) { return kLongCap; }

int64_t lcfe_gp2d_max_points(void) { return kGpLongNP - 1; }

int64_t lcfe_gp1d_max_points(void) { return kGp1dLongTierNP - 1; }

int lcfe_implemented_mask(void) {
    int m = 0;
    for (int s = 0; s < NUM_SETS; ++s)
        if (set_implemented(s)) m |= 1 << s;
    return m;
}

int lcfe_implemented_xmask(void) {
    int m = 0;
    for (int s = NUM_SETS; s < NUM_SETS + LCFE_NUM_XSETS; ++s)
        if (set_implemented(s)) m |= 1 << s;
    return m;
}

int lcfe_set_count(void) {
    int n = 0;
    for (int s = 0; s < NUM_ALL_SETS; ++s) n += set_implemented(s) ? 1 : 0;
    return n;
}

int lcfe_set_info(int k, int* bit, const char** name, int* ncols, int* nstatus) {
    for (int s = 0; s < NUM_ALL_SETS; ++s) {
        if (!set_implemented(s) || k-- != 0) continue;
        if (bit) *bit = s;
        if (name) *name = set_name(s);
        if (ncols) *ncols = set_ncols(s);
        if (nstatus) *nstatus = set_nstatus(s);
        return 0;
    }
    return 1;
}

int lcfe_last_set_profile(int bit, double* kernel_ms, int32_t* launches) {
    if (!set_implemented(bit)) return 1;
    if (kernel_ms) *kernel_ms = g_set_ms[bit];
    if (launches) *launches = g_set_launches[bit];
    return 0;
}

int lcfe_last_ext_profile(double* kernel_ms, int32_t* launches, int n) {
    const int k = (n < LCFE_NUM_XSETS) ? ((n > 0) ? n : 0) : LCFE_NUM_XSETS;
    for (int x = 0; x < k; ++x) {
        if (kernel_ms) kernel_ms[x] = g_set_ms[NUM_SETS + x];
        if (launches) launches[x] = g_set_launches[NUM_SETS + x];
    }
    return LCFE_NUM_XSETS;
}

int64_t lcfe_ncols(int mask) {
    int64_t n = 0;
    for (int s = 0; s < NUM_ALL_SETS; ++s)
        if (mask & (1 << s)) n += set_ncols(s);
    return n;
}

int64_t lcfe_nstatus(int mask) {
    int64_t n = 0;
    for (int s = 0; s < NUM_ALL_SETS; ++s)
        if (mask & (1 << s)) n += set_nstatus(s);
    return n;
}

const char* lcfe_colname(int mask, int64_t j) {
    if (j < 0) return nullptr;
    for (int s = 0; s < NUM_ALL_SETS; ++s) {
        if (!(mask & (1 << s))) continue;
        if (j < set_ncols(s)) return kColNames[s][j];
        j -= set_ncols(s);
    }
    return nullptr;
}

// (layout: workspace.hpp)
size_t lcfe_workspace_bytes(int mask, int64_t n_obj, int64_t n_points) {
    return WsLayout(kWsSizes, mask, n_obj, n_points, 0, false).total;
}

size_t lcfe_workspace_bytes_for(int mask, int64_t n_obj, int64_t n_points, int64_t max_len) {
    return WsLayout(kWsSizes, mask, n_obj, n_points, max_len, true).total;
}

int lcfe_extract_device(int mask, int device, void* stream_, int64_t n_obj, int64_t n_points,
                        int64_t max_len, const int64_t* d_offsets, const double* d_t, const double* d_flux,
                        const double* d_err, const uint8_t* d_band, const double* d_z, double* d_out,
                        int32_t* d_status, void* d_workspace, size_t workspace_bytes, lcfe_stats* prof) {
    g_err.clear();
    if (mask <= 0 || mask >= (1 << NUM_ALL_SETS)) return fail_msg("lcfe_extract_device: empty or unknown feature-set mask");
    for (int s = 0; s < NUM_ALL_SETS; ++s)
        if ((mask & (1 << s)) && !set_implemented(s))
            return fail_msg("lcfe_extract_device: feature set " + std::to_string(s) + " is not built into this library");
    if (n_obj < 0 || n_points < 0 || max_len < 0) return fail_msg("lcfe_extract_device: negative size");
    if (n_obj > 0x7fffffff - kBinThreads) return fail_msg("lcfe_extract_device: more than 2^31 objects in one batch");
    // fit ids are packed into int32: object * 8 + band (Bazin), object * 32 + band * 9 + model (decline fits)
    if ((mask & (1 << SET_BAZIN)) && n_obj >= (1ll << 28))
        return fail_msg("lcfe_extract_device: the Bazin set takes fewer than 2^28 objects per batch (split the batch)");
    if ((mask & (1 << SET_POWERLAW)) && n_obj >= (1ll << 26))
        return fail_msg("lcfe_extract_device: the power-law set takes fewer than 2^26 objects per batch (split the batch)");
    if (n_obj == 0) return 0;
    if (!d_offsets || !d_out || (n_points > 0 && (!d_t || !d_flux || !d_err || !d_band)))
        return fail_msg("lcfe_extract_device: null array");
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg("lcfe_extract_device: cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    hipStream_t stream = (hipStream_t)stream_;
    BatchView B{d_offsets, d_t, d_flux, d_err, d_band, d_z, n_obj};
    const int ld = (int)lcfe_ncols(mask);
    const int st_ld = (int)lcfe_nstatus(mask);
    if (prof) {
        memset(prof, 0, sizeof *prof);
        for (int s = 0; s < NUM_ALL_SETS; ++s) { g_set_ms[s] = 0; g_set_launches[s] = 0; }
        prof->bytes_in = 25 * n_points + 8 * (n_obj + 1) + (d_z ? 8 * n_obj : 0);
        prof->bytes_out = 8 * n_obj * (int64_t)ld;
    }
    const WsLayout L(kWsSizes, mask, n_obj, n_points, max_len, true);
    if (!d_workspace || workspace_bytes < L.short_total)
        return fail_msg("lcfe_extract_device: workspace smaller than lcfe_workspace_bytes(mask, n_obj, n_points)");
    unsigned long long* tickets = (unsigned long long*)d_workspace;
    int* counts = (int*)((char*)d_workspace + kWsCounts);
    int* lists = (int*)L.at(d_workspace, WS_LISTS);
    double* gp_slab[kGpNumTiers];
    for (int k = 0; k < kGpNumTiers; ++k) gp_slab[k] = (double*)L.at(d_workspace, WS_GP_TIER + k);
    // the slabs of the long-object tier, when the workspace was sized with lcfe_workspace_bytes_for(.., max_len)
    char* long_slab[NUM_ALL_SETS] = {};
    if (workspace_bytes >= L.total)
        for (int s = 0; s < NUM_ALL_SETS; ++s)
            if (L.bytes[WS_LONG + s]) long_slab[s] = L.at(d_workspace, WS_LONG + s);
    const Bins bins{lists, counts, n_obj};
    // Launch plan.  The sets write disjoint columns and only read the bins, so after the shared prologue
    // (+ the statistics set, which stays alone so that its event time is a clean roofline sample) the
    // remaining sets are enqueued on side streams forked from the caller's stream and joined back
    // into it: the heavy-tailed end of one kernel is filled by the workgroups of another, and the
    // register-bound fit kernels (1-2 waves per SIMD) share the SIMDs with each other.
    // LCFE_SERIAL=1 keeps everything on the caller's stream (per-set times then do not overlap).
    static const bool serial = [] { const char* e = getenv("LCFE_SERIAL"); return e && e[0] == '1'; }();
    hipStream_t side[kSideStreams];
    const bool fork = !serial && side_streams(dev, side) == 0;
    // timing events (prof only): created once per host thread and device, reused by later calls -- a call with
    // `prof` drains the stream before it returns, so the events of the previous call are always complete
    struct Events {
        hipEvent_t ev0[NUM_ALL_SETS] = {}, ev1[NUM_ALL_SETS] = {};
        bool ready = false;
    };
    static thread_local Events pools[16];
    Events& E = pools[(dev >= 0 && dev < 16) ? dev : 0];
    hipEvent_t (&ev0)[NUM_ALL_SETS] = E.ev0;
    hipEvent_t (&ev1)[NUM_ALL_SETS] = E.ev1;
    // (the one marker several streams wait on; every other fork and join is a stream_wait)
    struct Marker {
        hipEvent_t e = nullptr;
        ~Marker() { if (e) (void)hipEventDestroy(e); }
    } fork_marker;
    hipEvent_t& forked = fork_marker.e;
    if (prof && !E.ready) {
        for (int k = 0; k < NUM_ALL_SETS; ++k) { HIP_TRY(hipEventCreate(&ev0[k])); HIP_TRY(hipEventCreate(&ev1[k])); }
        E.ready = true;
    }
    bool side_used[kSideStreams] = {false, false, false, false, false};
    int col0 = 0, st0 = 0, ne = 0;
    for (int s = 0; s < NUM_ALL_SETS; ++s) {
        if (!(mask & (1 << s))) continue;
        if (ne == 0) {
            // shared prologue (timed with the first set): zero tickets and counts, bin the objects
            if (prof) HIP_TRY(hipEventRecord(ev0[s], stream));
            HIP_TRY(hipMemsetAsync(d_workspace, 0, kWsHeader, stream));
            hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((n_obj + kBinThreads - 1) / kBinThreads)), dim3(kBinThreads), 0,
                               stream, d_offsets, n_obj, lists, counts);
            HIP_TRY(hipGetLastError());
        }
        // stream of the set (SetTraits::stream): the 2-D GP (the longest) and the statistics stay on the caller's stream
        const int side_k = for_set(s, [](auto tag) { return SetTraits<tag()>::stream; }, int(STREAM_CALLER));
        hipStream_t q = (fork && side_k >= 0) ? side[side_k] : stream;
        if (fork && s != SET_STAT && !forked) {
            HIP_TRY(hipEventCreateWithFlags(&forked, hipEventDisableTiming));
            HIP_TRY(hipEventRecord(forked, stream));
        }
        if (q != stream) {
            if (!side_used[side_k]) { HIP_TRY(hipStreamWaitEvent(q, forked, 0)); side_used[side_k] = true; }
        }
        if (prof && ne != 0) HIP_TRY(hipEventRecord(ev0[s], q));
        int nl = 0;
        const SetLaunch A{B, bins, max_len, SetOut{d_out, ld, col0, d_status, st_ld, st0}, q, dev, &nl, tickets, long_slab[s]};
        const int rc = for_set(s, [&](auto tag) -> int {
            constexpr int SET = tag();
            if constexpr (SET == SET_STAT) return A.launch_stat(fork ? side[0] : q, fork ? side[1] : q);
            else if constexpr (SET == SET_BAZIN) return A.launch_fits<BazinFits>(bazin_ws(L, d_workspace));
            else if constexpr (SET == SET_POWERLAW) return A.launch_fits<DeclineFits>(powerlaw_ws(L, d_workspace));
            else if constexpr (SET == SET_GP1D) return A.launch_gp1d((double*)L.at(d_workspace, WS_GP1D));
            else if constexpr (SET == SET_GP2D) {
                // the GP tiers, longest first, round-robin over the caller's stream and side streams 2.. (LCFE_GP_STREAMS, default
                // 2: more streams start more tiers at once)
                static const int want = [] { const char* e = getenv("LCFE_GP_STREAMS"); const int k = e ? atoi(e) : 2; return (k < 1) ? 1 : ((k > 4) ? 4 : k); }();
                hipStream_t gs[4] = {q, q, q, q};
                int ngs = 1;
                if (fork) {
                    for (int k = 1; k < want; ++k) {
                        gs[k] = side[1 + k];
                        if (!side_used[1 + k]) { HIP_TRY(hipStreamWaitEvent(side[1 + k], forked, 0)); side_used[1 + k] = true; }
                    }
                    ngs = want;
                }
                int rc = A.launch_gp(gs, ngs, gp_slab);
                // the set's stop event (prof) is recorded on q: make q wait for the tiers on the other streams
                for (int k = 1; k < ngs && !rc; ++k) rc = stream_wait(q, gs[k]);
                return rc;
            } else return A.template launch_set<SET>();
        });
        if (rc) return rc;
        if (prof) {
            HIP_TRY(hipEventRecord(ev1[s], q));
            if (s < NUM_SETS) prof->launches[s] = nl;
            g_set_launches[s] = nl;
        }
        ++ne;
        col0 += set_ncols(s);
        st0 += set_nstatus(s);
    }
    // join the side streams back into the caller's stream
    for (int k = 0; k < kSideStreams; ++k) {
        if (side_used[k] && stream_wait(stream, side[k])) return 1;
    }
    if (prof) {
        HIP_TRY(hipStreamSynchronize(stream));
        for (int s = 0; s < NUM_ALL_SETS; ++s) {
            if (!(mask & (1 << s))) continue;
            float ms = 0;
            HIP_TRY(hipEventElapsedTime(&ms, ev0[s], ev1[s]));
            if (s < NUM_SETS) prof->kernel_ms[s] = ms;
            g_set_ms[s] = ms;
        }
    }
    return 0;
}

int lcfe_extract(int mask, int device, int64_t n_obj, const int64_t* offsets, const double* t,
                 const double* flux, const double* err, const uint8_t* band, const double* z, double* out,
                 int32_t* status, lcfe_stats* prof) {
    g_err.clear();
    if (n_obj < 0) return fail_msg("lcfe_extract: negative n_obj");
    if (n_obj == 0) return 0;
    if (!offsets || !out) return fail_msg("lcfe_extract: null array");
    if (lcfe_device_count() < 1) return fail_msg("lcfe_extract: no HIP device visible (liblcfe has no CPU fallback)");
    // host-side validation: a malformed CSR must never reach a kernel
    if (offsets[0] != 0) return fail_msg("lcfe_extract: offsets[0] != 0");
    int64_t max_len = 0;
    for (int64_t i = 0; i < n_obj; ++i) {
        const int64_t n = offsets[i + 1] - offsets[i];
        if (n < 0) return fail_msg("lcfe_extract: offsets not non-decreasing");
        if (n > max_len) max_len = n;
    }
    const int64_t np = offsets[n_obj];
    if (np > 0 && (!t || !flux || !err || !band)) return fail_msg("lcfe_extract: null sample array");
    const int64_t ld = lcfe_ncols(mask), st_ld = lcfe_nstatus(mask);
    if (ld <= 0) return fail_msg("lcfe_extract: empty feature-set mask");
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg("lcfe_extract: cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 16) return fail_msg("lcfe_extract: device index out of range");
    // Per-device pool of staging buffers and events, grown on demand and kept for the life of the process: a
    // statistics-only call used to spend 27 of its 38 ms in nine hipMalloc/hipFree pairs.  One host-buffer call
    // at a time per device holds the pool (concurrent callers on one device are serialised here).
    HostPathPool& P = g_pool[dev];
    std::lock_guard<std::mutex> pool_lock(P.mutex);
    const size_t npa = (size_t)(np > 0 ? np : 1);
    const size_t wsb = lcfe_workspace_bytes_for(mask, n_obj, np, max_len);
    const size_t need[HostPathPool::NBUF] = {sizeof(int64_t) * (size_t)(n_obj + 1), 8 * npa, 8 * npa, 8 * npa, npa,
                                             z ? 8 * (size_t)n_obj : 0, 8 * (size_t)n_obj * (size_t)ld,
                                             st_ld > 0 ? 4 * (size_t)n_obj * (size_t)st_ld : 0, wsb};
    for (int k = 0; k < HostPathPool::NBUF; ++k) {
        if (need[k] <= P.cap[k]) continue;
        if (P.buf[k]) { (void)hipFree(P.buf[k]); P.buf[k] = nullptr; P.cap[k] = 0; }
        const size_t want = need[k] + need[k] / 4;               // head room: batches of similar size reuse the block
        hipError_t e = hipMalloc(&P.buf[k], want);
        if (e != hipSuccess) { e = hipMalloc(&P.buf[k], need[k]); if (e == hipSuccess) P.cap[k] = need[k]; }
        else P.cap[k] = want;
        if (e != hipSuccess) return fail("hipMalloc(host-path pool)", e, __FILE__, __LINE__);
    }
    for (int k = 0; k < 4; ++k)
        if (!P.ev[k]) HIP_TRY(hipEventCreate(&P.ev[k]));
    int64_t* d_off = (int64_t*)P.buf[0];
    double *d_t = (double*)P.buf[1], *d_f = (double*)P.buf[2], *d_e = (double*)P.buf[3];
    uint8_t* d_b = (uint8_t*)P.buf[4];
    double* d_z = z ? (double*)P.buf[5] : nullptr;
    double* d_out = (double*)P.buf[6];
    int32_t* d_st = st_ld > 0 ? (int32_t*)P.buf[7] : nullptr;
    void* d_ws = P.buf[8];
    HIP_TRY(hipEventRecord(P.ev[0], 0));
    HIP_TRY(hipMemcpyAsync(d_off, offsets, sizeof(int64_t) * (n_obj + 1), hipMemcpyHostToDevice, 0));
    if (np > 0) {
        HIP_TRY(hipMemcpyAsync(d_t, t, 8 * np, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(d_f, flux, 8 * np, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(d_e, err, 8 * np, hipMemcpyHostToDevice, 0));
        HIP_TRY(hipMemcpyAsync(d_b, band, np, hipMemcpyHostToDevice, 0));
    }
    if (z) HIP_TRY(hipMemcpyAsync(d_z, z, 8 * n_obj, hipMemcpyHostToDevice, 0));
    if (d_st) HIP_TRY(hipMemsetAsync(d_st, 0, 4 * (size_t)n_obj * st_ld, 0));
    HIP_TRY(hipEventRecord(P.ev[1], 0));
    lcfe_stats local;
    const int rc = lcfe_extract_device(mask, -1, nullptr, n_obj, np, max_len, d_off, d_t, d_f, d_e, d_b, d_z, d_out, d_st,
                                       d_ws, wsb, prof ? &local : nullptr);
    if (rc) { (void)hipStreamSynchronize(0); return rc; }
    HIP_TRY(hipEventRecord(P.ev[2], 0));
    HIP_TRY(hipMemcpyAsync(out, d_out, 8 * (size_t)n_obj * ld, hipMemcpyDeviceToHost, 0));
    if (status && d_st) HIP_TRY(hipMemcpyAsync(status, d_st, 4 * (size_t)n_obj * st_ld, hipMemcpyDeviceToHost, 0));
    HIP_TRY(hipEventRecord(P.ev[3], 0));
    HIP_TRY(hipStreamSynchronize(0));
    if (prof) {
        *prof = local;
        float ms = 0;
        (void)hipEventElapsedTime(&ms, P.ev[0], P.ev[1]); prof->h2d_ms = ms;
        (void)hipEventElapsedTime(&ms, P.ev[2], P.ev[3]); prof->d2h_ms = ms;
    }
    return 0;
}

/* release the staging buffers lcfe_extract keeps per device (optional; they are reused by later calls) */
void lcfe_release_buffers(void) {
    for (int d = 0; d < 16; ++d) {
        HostPathPool& P = g_pool[d];
        std::lock_guard<std::mutex> lock(P.mutex);
        bool any = false;
        for (int k = 0; k < HostPathPool::NBUF; ++k) any = any || P.buf[k];
        if (!any) continue;
        DeviceGuard guard;
        if (guard.enter(d)) continue;
        for (int k = 0; k < HostPathPool::NBUF; ++k) { if (P.buf[k]) (void)hipFree(P.buf[k]); P.buf[k] = nullptr; P.cap[k] = 0; }
    }
}

int64_t lcfe_augment_capacity(int64_t n_points, int k) {
    if (n_points < 0 || k < 1 || n_points > INT64_MAX / k) return -1;
    return n_points * k;
}

size_t lcfe_augment_workspace_bytes(int64_t n_obj, int k) {
    if (n_obj < 0 || k < 1 || n_obj > (INT64_MAX >> 4) / k) return 0;
    return AugWs(nullptr, n_obj, k).bytes;
}

int lcfe_augment_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int k, const int64_t* d_offsets,
                        const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, const double* d_scale,
                        const double* d_stretch, const double* d_shift, const double* d_noise_scale, const double* d_dropout,
                        const uint8_t* d_band_noise, const uint64_t* d_seed, const double* d_add_flux, const uint8_t* d_keep,
                        int64_t* d_offsets_out, double* d_t_out, double* d_flux_out, double* d_err_out, uint8_t* d_band_out,
                        int64_t* d_n_points_out, void* d_workspace, size_t workspace_bytes) {
    const AugIn A{d_offsets, d_t, d_flux, d_err, d_band, d_add_flux, d_keep, k, nullptr};
    const AugPlan P{d_scale, d_stretch, d_shift, d_noise_scale, d_dropout, d_band_noise, d_seed, nullptr, nullptr, nullptr, AUG_KEEP_FLOOR5};
    const AugOut O{d_offsets_out, d_t_out, d_flux_out, d_err_out, d_band_out};
    return augment_launch<false>("lcfe_augment_device", device, stream_, n_obj, n_points, k, A, P, O, d_n_points_out, d_workspace,
                                 workspace_bytes);
}

int lcfe_augment_recipe_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int k, const int64_t* d_offsets,
                               const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band,
                               const double* d_scale, const double* d_stretch, const double* d_shift, const double* d_noise_scale,
                               const double* d_dropout, const uint8_t* d_band_noise, const uint64_t* d_seed,
                               const double* d_band_scale, const double* d_err_boost, const double* d_noise2_scale, int keep_rule,
                               const double* d_add_flux, const uint8_t* d_keep, const double* d_add_flux2, int64_t* d_offsets_out,
                               double* d_t_out, double* d_flux_out, double* d_err_out, uint8_t* d_band_out, int64_t* d_n_points_out,
                               void* d_workspace, size_t workspace_bytes) {
    const AugIn A{d_offsets, d_t, d_flux, d_err, d_band, d_add_flux, d_keep, k, d_add_flux2};
    const AugPlan P{d_scale, d_stretch, d_shift, d_noise_scale, d_dropout, d_band_noise, d_seed, d_band_scale, d_err_boost,
                    d_noise2_scale, keep_rule};
    const AugOut O{d_offsets_out, d_t_out, d_flux_out, d_err_out, d_band_out};
    return augment_launch<true>("lcfe_augment_recipe_device", device, stream_, n_obj, n_points, k, A, P, O, d_n_points_out,
                                d_workspace, workspace_bytes);
}

size_t lcfe_sequences_workspace_bytes(int64_t n_obj, int64_t n_points, int64_t max_len) {
    (void)n_obj; (void)n_points; (void)max_len;
    return 0;                               // every pass streams from the batch
}

int lcfe_sequences_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int64_t max_length, int normalize,
                          const int64_t* d_offsets, const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band,
                          float* d_features, int64_t* d_bands, float* d_mask, int64_t* d_length, float* d_mean, float* d_std,
                          void* d_workspace, size_t workspace_bytes) {
    g_err.clear();
    if (max_length < 1) return fail_msg("lcfe_sequences_device: max_length must be at least 1");
    if (n_obj < 0 || n_points < 0) return fail_msg("lcfe_sequences_device: negative size");
    if (n_obj > (INT64_MAX >> 5) / max_length) return fail_msg("lcfe_sequences_device: n_obj * max_length overflows");
    if (!d_offsets) return fail_msg("lcfe_sequences_device: null offsets");
    if (n_points > 0 && (!d_t || !d_flux || !d_err || !d_band)) return fail_msg("lcfe_sequences_device: null sample array");
    if (n_obj > 0 && (!d_features || !d_bands || !d_mask || !d_length || !d_mean || !d_std))
        return fail_msg("lcfe_sequences_device: null output array");
    if ((uintptr_t)d_features & 15) return fail_msg("lcfe_sequences_device: features must be aligned to 16 bytes");
    const size_t need = lcfe_sequences_workspace_bytes(n_obj, n_points, 0);
    if (need > 0 && (!d_workspace || workspace_bytes < need))
        return fail_msg("lcfe_sequences_device: workspace smaller than lcfe_sequences_workspace_bytes(n_obj, n_points, max_len)");
    if (n_obj == 0) return 0;
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg("lcfe_sequences_device: cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const SeqIn A{d_offsets, d_t, d_flux, d_err, d_band};
    const SeqOut O{reinterpret_cast<SeqRow*>(d_features), d_bands, d_mask, d_length, d_mean, d_std};
    const int64_t groups = (n_obj + kSeqWaves - 1) / kSeqWaves, cap = (int64_t)num_cus(dev) * 8;
    const unsigned grid = (unsigned)((groups < cap) ? groups : cap);
    hipLaunchKernelGGL(sequences_kernel, dim3(grid), dim3(64 * kSeqWaves), 0, (hipStream_t)stream_, A, O, n_obj, max_length, normalize);
    HIP_TRY(hipGetLastError());
    return 0;
}

int64_t lcfe_gp2d_grid_max_times(void) { return GP_GRID_MAX_TIMES; }

// (the gp2d set's own workspace: header, index lists, the tiers' Gram-matrix slabs, the long-object tier's slabs)
size_t lcfe_gp2d_grid_workspace_bytes(int64_t n_obj, int64_t n_points, int64_t max_len) {
    return lcfe_workspace_bytes_for(1 << SET_GP2D, n_obj, n_points, max_len);
}

int lcfe_gp2d_grid_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                          const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int n_times,
                          const double* d_grid_offsets, int origin, int n_bands, const int* bands, const double* d_theta_in,
                          double* d_mean, double* d_var, double* d_theta_out, double* d_row27, int32_t* d_status, void* d_workspace,
                          size_t workspace_bytes) {
    g_err.clear();
    const char* me = "lcfe_gp2d_grid_device: ";
    if (n_times < 1 || n_times > GP_GRID_MAX_TIMES)
        return fail_msg(std::string(me) + "n_times must lie in [1, " + std::to_string(GP_GRID_MAX_TIMES) + "]");
    if (n_bands < 1 || n_bands > GP_GRID_MAX_BANDS || !bands) return fail_msg(std::string(me) + "n_bands must lie in [1, 6]");
    unsigned codes = 0, seen = 0;
    for (int b = 0; b < n_bands; ++b) {
        if (bands[b] < 0 || bands[b] > 5) return fail_msg(std::string(me) + "a band outside 0..5");
        if (seen & (1u << bands[b])) return fail_msg(std::string(me) + "a band is listed twice");
        seen |= 1u << bands[b];
        codes |= (unsigned)bands[b] << (4 * b);
    }
    if (origin != LCFE_GRID_FROM_PEAK && origin != LCFE_GRID_FROM_FIRST) return fail_msg(std::string(me) + "unknown origin");
    if (n_obj < 0 || n_points < 0 || max_len < 0) return fail_msg(std::string(me) + "negative size");
    if (n_obj > 0x7fffffff - kBinThreads) return fail_msg(std::string(me) + "more than 2^31 objects in one batch");
    if (!d_offsets || !d_grid_offsets) return fail_msg(std::string(me) + "null offsets");
    if (n_points > 0 && (!d_t || !d_flux || !d_err || !d_band)) return fail_msg(std::string(me) + "null sample array");
    if (n_obj > 0 && (!d_mean || !d_theta_out || !d_status)) return fail_msg(std::string(me) + "null output array");
    if (d_theta_in && d_row27) return fail_msg(std::string(me) + "row27 is an output of fit mode (theta_in null)");
    if (n_obj == 0) return 0;
    const BatchView B{d_offsets, d_t, d_flux, d_err, d_band, nullptr, n_obj};
    const GpGridOut O{GpGridSpec{d_grid_offsets, n_times, n_bands, origin, codes}, d_theta_in, d_mean, d_var, d_theta_out, d_row27, d_status};
    return gp_grid_enqueue(me, device, (hipStream_t)stream_, n_obj, n_points, max_len, B, O, d_workspace, workspace_bytes);
}

size_t lcfe_gp2d_points_workspace_bytes_for(int64_t n_obj, int64_t n_points, int64_t max_len) {
    return lcfe_workspace_bytes_for(1 << SET_GP2D, n_obj, n_points, max_len);
}

int lcfe_gp2d_points_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                            const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int64_t nq,
                            const int64_t* d_q_off, const double* d_q_t, const double* d_q_lam, int origin, const double* d_theta_in,
                            int want_var, double* d_mean, double* d_var, double* d_theta_out, double* d_row27, int32_t* d_status,
                            void* d_workspace, size_t workspace_bytes) {
    g_err.clear();
    const char* me = "lcfe_gp2d_points_device: ";
    if (origin != LCFE_GRID_FROM_PEAK && origin != LCFE_GRID_FROM_FIRST) return fail_msg(std::string(me) + "unknown origin");
    if (n_obj < 0 || n_points < 0 || max_len < 0 || nq < 0) return fail_msg(std::string(me) + "negative size");
    if (n_obj > 0x7fffffff - kBinThreads) return fail_msg(std::string(me) + "more than 2^31 objects in one batch");
    if (!d_offsets || !d_q_off) return fail_msg(std::string(me) + "null offsets");
    if (n_points > 0 && (!d_t || !d_flux || !d_err || !d_band)) return fail_msg(std::string(me) + "null sample array");
    if (nq > 0 && (!d_q_t || !d_q_lam)) return fail_msg(std::string(me) + "null point array");
    if (n_obj > 0 && (!d_theta_out || !d_status)) return fail_msg(std::string(me) + "null output array");
    if (nq > 0 && (!d_mean || (want_var && !d_var))) return fail_msg(std::string(me) + "null output array");
    if (d_theta_in && d_row27) return fail_msg(std::string(me) + "row27 is an output of fit mode (theta_in null)");
    if (n_obj > 0 && (!d_workspace || workspace_bytes < lcfe_gp2d_points_workspace_bytes_for(n_obj, n_points, max_len)))
        return fail_msg(std::string(me) + "workspace smaller than lcfe_gp2d_points_workspace_bytes_for(n_obj, n_points, max_len)");
    // q_off lives on the device: ONE blocking copy of the whole array (8 (n_obj + 1) bytes) before anything is enqueued, so
    // that a list that is not ascending from 0 to nq, or an object with 2^31 points, is an error here and not an
    // out-of-bounds store there
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(std::string(me) + "cannot select device " + std::to_string(device));
    hipStream_t q = (hipStream_t)stream_;
    std::vector<int64_t> qo((size_t)n_obj + 1);
    HIP_TRY(hipMemcpyAsync(qo.data(), d_q_off, qo.size() * sizeof(int64_t), hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    if (qo[0] != 0) return fail_msg(std::string(me) + "q_off[0] must be 0");
    for (int64_t i = 0; i < n_obj; ++i) {
        if (qo[i + 1] < qo[i]) return fail_msg(std::string(me) + "q_off must not descend");
        if (qo[i + 1] - qo[i] > 0x7fffffff) return fail_msg(std::string(me) + "more than 2^31 points of one light curve");
    }
    if (qo[n_obj] != nq) return fail_msg(std::string(me) + "q_off[n_obj] must equal nq");
    if (n_obj == 0) return 0;
    const BatchView B{d_offsets, d_t, d_flux, d_err, d_band, nullptr, n_obj};
    const GpPointsOut O{d_q_off, d_q_t, d_q_lam, origin, d_theta_in, d_mean, want_var ? d_var : nullptr, d_theta_out, d_row27, d_status};
    return gp_grid_enqueue(me, device, q, n_obj, n_points, max_len, B, O, d_workspace, workspace_bytes);
}

// The per-band GP's posterior at a caller's times.  Workspace: the gp1d set's own (header, index lists, the slabs of the
// long bands and of the long-object tier), then the grouped query order (one int per query) and the groups' starts (five
// ints per light curve) -- sized by the queries' own count, not through the set masks.
static size_t gp1d_points_set_bytes(int64_t n_obj, int64_t n_points, int64_t max_len) {
    return WsLayout(kWsSizes, 1 << SET_GP1D, n_obj, n_points, max_len, true).total;
}
static size_t gp1d_points_perm_bytes(int64_t nq) { return (((size_t)(nq > 0 ? nq : 0) * sizeof(int)) + 255) & ~(size_t)255; }

size_t lcfe_gp1d_points_workspace_bytes_for(int64_t n_obj, int64_t n_points, int64_t max_len, int64_t nq) {
    return gp1d_points_set_bytes(n_obj, n_points, max_len) + gp1d_points_perm_bytes(nq) +
           (((size_t)(n_obj > 0 ? n_obj : 0) * 5 * sizeof(int) + 255) & ~(size_t)255);
}

int lcfe_gp1d_points_device(int device, void* stream_, int64_t n_obj, int64_t n_points, int64_t max_len, const int64_t* d_offsets,
                            const double* d_t, const double* d_flux, const double* d_err, const uint8_t* d_band, int64_t nq,
                            const int64_t* d_q_off, const double* d_q_t, const uint8_t* d_q_band, const double* d_theta_in,
                            double* d_mean, double* d_std, double* d_theta_out, double* d_norm, double* d_cols, int32_t* d_status,
                            void* d_workspace, size_t workspace_bytes) {
    g_err.clear();
    const char* me = "lcfe_gp1d_points_device: ";
    if (n_obj < 0 || n_points < 0 || max_len < 0 || nq < 0) return fail_msg(std::string(me) + "negative size");
    if (n_obj > 0x7fffffff - kBinThreads) return fail_msg(std::string(me) + "more than 2^31 objects in one batch");
    if (!d_offsets || !d_q_off) return fail_msg(std::string(me) + "null offsets");
    if (n_points > 0 && (!d_t || !d_flux || !d_err || !d_band)) return fail_msg(std::string(me) + "null sample array");
    if (nq > 0 && (!d_q_t || !d_q_band)) return fail_msg(std::string(me) + "null query array");
    if (n_obj > 0 && (!d_theta_out || !d_norm || !d_cols || !d_status)) return fail_msg(std::string(me) + "null output array");
    if (nq > 0 && (!d_mean || !d_std)) return fail_msg(std::string(me) + "null output array");
    if (n_obj > 0 && (!d_workspace || workspace_bytes < lcfe_gp1d_points_workspace_bytes_for(n_obj, n_points, max_len, nq)))
        return fail_msg(std::string(me) + "workspace smaller than lcfe_gp1d_points_workspace_bytes_for(n_obj, n_points, max_len, nq)");
    // q_off is read back once and checked before anything is enqueued (as lcfe_gp2d_points_device does): a list that is not
    // ascending from 0 to nq is an error here and not an out-of-bounds store there
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(std::string(me) + "cannot select device " + std::to_string(device));
    hipStream_t q = (hipStream_t)stream_;
    std::vector<int64_t> qo((size_t)n_obj + 1);
    HIP_TRY(hipMemcpyAsync(qo.data(), d_q_off, qo.size() * sizeof(int64_t), hipMemcpyDeviceToHost, q));
    HIP_TRY(hipStreamSynchronize(q));
    if (qo[0] != 0) return fail_msg(std::string(me) + "q_off[0] must be 0");
    for (int64_t i = 0; i < n_obj; ++i) {
        if (qo[i + 1] < qo[i]) return fail_msg(std::string(me) + "q_off must not descend");
        if (qo[i + 1] - qo[i] > 0x7fffffff) return fail_msg(std::string(me) + "more than 2^31 queries of one light curve");
    }
    if (qo[n_obj] != nq) return fail_msg(std::string(me) + "q_off[n_obj] must equal nq");
    if (n_obj == 0) return 0;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const WsLayout L(kWsSizes, 1 << SET_GP1D, n_obj, n_points, max_len, true);
    int* perm = (int*)((char*)d_workspace + L.total);
    int* qboff = (int*)((char*)perm + gp1d_points_perm_bytes(nq));
    unsigned long long* tickets = (unsigned long long*)d_workspace;
    const Bins bins{(int*)L.at(d_workspace, WS_LISTS), (int*)((char*)d_workspace + kWsCounts), n_obj};
    const BatchView B{d_offsets, d_t, d_flux, d_err, d_band, nullptr, n_obj};
    const SetOut O{d_cols, Gp1dPointsOut::kNcol, 0, d_status, GP1D_NSTATUS, 0};
    const Gp1dPointsOut po{d_q_off, d_q_t, perm, qboff, d_theta_in, d_mean, d_std, d_theta_out, d_norm};
    HIP_TRY(hipMemsetAsync(d_workspace, 0, kWsHeader, q));
    hipLaunchKernelGGL(bin_kernel, dim3((unsigned)((n_obj + kBinThreads - 1) / kBinThreads)), dim3(kBinThreads), 0, q, d_offsets, n_obj,
                       bins.lists, bins.counts);
    HIP_TRY(hipGetLastError());
    const int64_t cap = (int64_t)num_cus(dev) * 8;
    const int64_t groups = std::min<int64_t>((n_obj + kGp1dGroupWaves - 1) / kGp1dGroupWaves, cap);
    hipLaunchKernelGGL(gp1d_group_queries_kernel, dim3((unsigned)groups), dim3(64 * kGp1dGroupWaves), 0, q, d_q_off, d_q_band, n_obj, perm, qboff);
    HIP_TRY(hipGetLastError());
    // every output a band may leave alone is NaN first: queries of a band without a fit, with a code outside 1..4 or of a
    // light curve no tier takes; theta and norm of such bands
    const struct { double* p; int64_t n; } fills[] = {{d_mean, nq}, {d_std, nq}, {d_theta_out, n_obj * GP1D_NBAND * GP1D_NTHETA},
                                                    {d_norm, n_obj * GP1D_NBAND * GP1D_NNORM}};
    for (const auto& f : fills) {
        if (f.n < 1) continue;
        hipLaunchKernelGGL(gp1d_points_nan_kernel, dim3((unsigned)std::min<int64_t>((f.n + 255) / 256, cap)), dim3(256), 0, q, f.p, f.n);
        HIP_TRY(hipGetLastError());
    }
    // the tiers as SetLaunch::launch_gp1d runs them: every band in its row capacity, on the caller's stream
    double* kslab = (double*)L.at(d_workspace, WS_GP1D);
    const int last = gp_last_tier(max_len);
    for (int ti = last; ti >= 0; --ti) {
        const int nan_from = nan_from_of(ti, last);
        int rc = 0;
        switch ((ti < kGp1dKernelTiers) ? ti : kGp1dKernelTiers - 1) {
#define X(id, NP, ROWCAP, WNP, MW)                                                                                                          \
    case id:                                                                                                                                \
        rc = launch_grid(gp1d_points_kernel<NP, ROWCAP, kGp1dThreads, WNP, MW>, kGp1dThreads, {0, (ROWCAP > NP) ? kGp1dLongGrid : 0}, n_obj, 1, q, \
                         dev, B, bins, ti, nan_from, O, tickets + SET_GP1D * 8 + ti, (ROWCAP > NP) ? kslab : nullptr, po);                 \
        break;
            LCFE_GP1D_KERNEL_TIERS(X)
#undef X
        }
        if (rc) return rc;
    }
    if (L.bytes[WS_LONG + SET_GP1D] && max_len > SetTraits<SET_GP1D>::long_above) {
        hipLaunchKernelGGL(gp1d_points_long_kernel, dim3(kGp1dLongTierGrid), dim3(kGp1dThreads), 0, q, B, bins, O, L.at(d_workspace, WS_LONG + SET_GP1D),
                           tickets + SET_GP1D * 8 + 7, po);
        HIP_TRY(hipGetLastError());
    }
    return 0;
}

int lcfe_gp_resample_query_device(int device, void* stream_, int64_t n_src, int k, int origin, const int64_t* d_offsets, const double* d_t,
                                  const double* d_flux, const double* d_err, const uint8_t* d_band, const double* d_z_old,
                                  const int64_t* d_copy_offsets, const double* d_copy_t, const uint8_t* d_copy_band, const double* d_z_new,
                                  const double* d_shift, int64_t* d_q_off, double* d_q_t, double* d_q_lam) {
    g_err.clear();
    const char* me = "lcfe_gp_resample_query_device: ";
    if (k < 1) return fail_msg(std::string(me) + "k must be at least 1");
    if (n_src < 0) return fail_msg(std::string(me) + "negative size");
    if (origin != LCFE_GRID_FROM_PEAK && origin != LCFE_GRID_FROM_FIRST) return fail_msg(std::string(me) + "unknown origin");
    if (!d_offsets || !d_copy_offsets || !d_q_off) return fail_msg(std::string(me) + "null offsets");
    if (n_src > 0 && (!d_t || !d_flux || !d_err || !d_band || !d_z_old || !d_copy_t || !d_copy_band || !d_z_new || !d_shift || !d_q_t || !d_q_lam))
        return fail_msg(std::string(me) + "null array");
    if (n_src == 0) return 0;
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(std::string(me) + "cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const GpResSource S{d_offsets, d_t, d_flux, d_err, d_band, d_z_old};
    const GpResCopies C{d_copy_offsets, d_copy_t, nullptr, d_copy_band, k};
    const GpResPlan P{d_z_new, nullptr, nullptr, d_shift, nullptr};
    const int64_t blocks = std::min<int64_t>((n_src + kAugWaves - 1) / kAugWaves, (int64_t)num_cus(dev) * 8);
    hipLaunchKernelGGL(gp_resample_query_kernel, dim3((unsigned)blocks), dim3(64 * kAugWaves), 0, (hipStream_t)stream_, S, C, P, n_src, origin,
                       d_q_off, d_q_t, d_q_lam);
    HIP_TRY(hipGetLastError());
    return 0;
}

int lcfe_gp_resample_write_device(int device, void* stream_, int64_t n_copies, int k, const int64_t* d_copy_offsets, const double* d_copy_err,
                                  const double* d_mean, const double* d_var, const double* d_dim, const double* d_noise, const uint64_t* d_seed,
                                  const double* d_n1, const double* d_n2, const int32_t* d_src_status, int n_status, double* d_flux_out,
                                  double* d_err_out, int32_t* d_status_out) {
    g_err.clear();
    const char* me = "lcfe_gp_resample_write_device: ";
    if (k < 1) return fail_msg(std::string(me) + "k must be at least 1");
    if (n_copies < 0 || n_copies % k != 0) return fail_msg(std::string(me) + "n_copies must be a multiple of k");
    if (n_status < 1) return fail_msg(std::string(me) + "n_status must be at least 1");
    if ((d_n1 == nullptr) != (d_n2 == nullptr)) return fail_msg(std::string(me) + "n1 and n2 come together (explicit mode) or not at all");
    if (!d_n1 && !d_seed) return fail_msg(std::string(me) + "Philox mode needs the seeds");
    if (!d_copy_offsets || !d_copy_err || !d_mean || !d_var || !d_dim || !d_noise || !d_src_status || !d_flux_out || !d_err_out || !d_status_out)
        return fail_msg(std::string(me) + "null array");
    if (n_copies == 0) return 0;
    DeviceGuard guard;
    if (guard.enter(device)) return fail_msg(std::string(me) + "cannot select device " + std::to_string(device));
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    const GpResCopies C{d_copy_offsets, nullptr, d_copy_err, nullptr, k};
    const GpResPlan P{nullptr, d_dim, d_noise, nullptr, d_seed ? d_seed : (const uint64_t*)d_dim};
    const int64_t blocks = std::min<int64_t>((n_copies + kAugWaves - 1) / kAugWaves, (int64_t)num_cus(dev) * 8);
    hipLaunchKernelGGL(gp_resample_write_kernel, dim3((unsigned)blocks), dim3(64 * kAugWaves), 0, (hipStream_t)stream_, C, P, n_copies, d_mean, d_var,
                       d_n1, d_n2, d_src_status, n_status, d_flux_out, d_err_out, d_status_out);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // extern "C"
