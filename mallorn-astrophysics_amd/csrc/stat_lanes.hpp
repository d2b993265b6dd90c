// stat_lanes.hpp -- statistics with SEVERAL light curves per wavefront and the bands in lanes of their own.
//
// The one-object-per-wavefront kernels (stat_lean.hpp) spend most of their instructions on things that
// are not statistics: cross-lane partner fetches of the sorting networks, 15 DPP reductions per group,
// padding of 23-row bands to 32 slots in 8 of 64 lanes.  Here a light curve owns a group of LPO lanes and a
// BAND OWNS ITS LANES: the band's fluxes sit in those lanes' registers, the moment passes are plain serial
// loops without any reduction, the band sort is a sorting network on registers (v_min/v_max pairs, no
// partner fetch) and all light curves of the wavefront share every instruction.  A band is split in time over
// its lanes (its "parts"), r and i -- the two long bands of the survey's cadence -- over twice as many as the
// others, so that a register array of CAP values holds bands of parts x CAP rows.  The two layouts
// (LanesLayout<LPO>):
//
//   LPO = 8, eight light curves per wavefront: u, g, z, y one lane (CAP rows), r and i two (2 CAP rows)
//     lane of the group   0   1   2        3         4   5   6        7
//     rows                u   g   r first  r second  z   y   i first  i second
//
//   LPO = 16, four light curves per wavefront: u, g, z, y two lanes (2 CAP rows), r and i four (4 CAP rows) -- a lane
//   takes 1/16 of the rows, so light curves of up to 512 rows keep the register and LDS footprint of LPO = 8 at 256
//     lane of the group   0  1   2  3   4  5  6  7   8  9   10 11   12 13 14 15
//     rows                u  u   g  g   r  r  r  r   z  z   y  y    i  i  i  i
//
// One workgroup (= one wavefront) takes one batch of 64 / LPO light curves; lane j of a group first holds rows j,
// j + LPO, ... of its light curve (t, f, e, band code) in registers from ONE round of loads.  Phases (one LDS buffer of
// 64 columns x (CAP + 1) doubles per wavefront, reused):
//   A  positions: a row's slot = number of earlier rows of its band (ballots over the LPO rows of a trip); per row also
//      the all-rows slope and the "rows ascend in time" check from the file-order neighbours (next lane / next trip)
//      and the SNR term |f| / e
//   F  fluxes -> LDS (column = lane that owns the part of the band) -> registers v[0..CAP); sums, NaN flags
//   T  times  -> LDS -> band slopes against the register-resident fluxes
//   Q  SNR terms -> LDS -> sums
//   then the two centred passes (band and all-rows moments side by side, select-free on a copy padded with the band
//   mean; a band's sums are combined over its lanes, the all-rows sums over the group), the register sort, and a
//   bitonic MERGE of the sorted lanes, level by level: a band of P parts is complete after log2(P) levels, the light
//   curve after log2(LPO).  Extrema and order statistics are read off the LDS dump of the level that completes their
//   sequence by one lane per sequence; the all-rows columns are parked in LDS as they get ready (the kernel has no
//   register to spare).
// Which light curves come here is decided by stat_plan_kernel (lcfe.hip) from the rows per band; a light curve whose
// rows turn out not to ascend in time is appended to the general kernel's list.  Same arithmetic per element as
// stat.hpp (two-pass moments, exact counts, numpy's percentile interpolation, exact MAD); the sums are associated
// differently, and the slope quotients go through the reciprocal (stat_slope).
#pragma once
#include <utility>
#include "stat.hpp"

namespace lcfe {

// Batcher's odd-even merge sort for N = 2^k keys as a compile-time list of compare-exchanges
// (63 / 191 / 543 for 16 / 32 / 64 keys; the bitonic network needs 80 / 240 / 672).
template <int N>
struct OddEvenNet {
    int count;
    unsigned char a[N * 10], b[N * 10];
    constexpr OddEvenNet() : count(0), a{}, b{} {
        for (int p = 1; p < N; p *= 2)
            for (int k = p; k >= 1; k /= 2)
                for (int j = k % p; j <= N - 1 - k; j += 2 * k)
                    for (int i = 0; i <= ((k - 1 < N - j - k - 1) ? k - 1 : N - j - k - 1); ++i)
                        if ((i + j) / (p * 2) == (i + j + k) / (p * 2)) {
                            a[count] = (unsigned char)(i + j);
                            b[count] = (unsigned char)(i + j + k);
                            ++count;
                        }
    }
};
template <int N>
inline constexpr OddEvenNet<N> kOddEvenNet{};

}  // namespace lcfe

#if defined(__HIPCC__)
namespace lcfe {
// reductions over the 16 lanes of a DPP row (= one light curve's group): every lane gets the result
struct Lanes16 {
    template <class V, class Op>
    static __device__ __forceinline__ V reduce(V v, Op op) {
        v = op(v, WaveDev::dpp<0xB1>(v));      // quad_perm(1,0,3,2)
        v = op(v, WaveDev::dpp<0x4E>(v));      // quad_perm(2,3,0,1)
        v = op(v, WaveDev::dpp<0x141>(v));     // row_half_mirror
        v = op(v, WaveDev::dpp<0x140>(v));     // row_mirror
        return v;
    }
    static __device__ __forceinline__ double sum(double v) { return reduce(v, [](double a, double b) { return a + b; }); }
    static __device__ __forceinline__ double max(double v) { return reduce(v, [](double a, double b) { return (b > a) ? b : a; }); }
    static __device__ __forceinline__ double min(double v) { return reduce(v, [](double a, double b) { return (b < a) ? b : a; }); }
    static __device__ __forceinline__ int sum(int v) { return reduce(v, [](int a, int b) { return a + b; }); }
    static __device__ __forceinline__ int max(int v) { return reduce(v, [](int a, int b) { return (b > a) ? b : a; }); }
    static __device__ __forceinline__ int min(int v) { return reduce(v, [](int a, int b) { return (b < a) ? b : a; }); }
    static __device__ __forceinline__ bool any(bool p) { return max(p ? 1 : 0) != 0; }
    static __device__ __forceinline__ bool all(bool p) { return min(p ? 1 : 0) != 0; }
    static __device__ __forceinline__ void sync() { GroupDev<8>::sync(); }
};
}  // namespace lcfe
#endif

namespace lcfe {

// ---- who holds what: LPO lanes per light curve.  band_of / first_lane / parts are the lane -> band table, the band ->
// first-lane table and the lanes ("parts", a power of two) a band is split over in time; G the reductions over the
// group; WRAP_DPP the DPP control with which the last lane of a group reads the first (the file-order neighbour of its
// row is in the next trip); ALL_ROWS_LANE the lane that writes the all-rows columns -- one that reads no band's order
// statistics.  A 32-lane layout would be a third specialisation (and reductions over two DPP rows).
constexpr int kLanesBands = 6;
template <int LANES_PER_OBJECT>
struct LanesLayout;
template <>
struct LanesLayout<8> {
    static constexpr int LPO = 8, MAX_PARTS = 2, ALL_ROWS_LANE = 3, WRAP_DPP = 0x117;        // row_shr:7
    static constexpr int band_of(int lane) { constexpr int t[LPO] = {0, 1, 2, 2, 4, 5, 3, 3}; return t[lane]; }
    static constexpr int first_lane(int band) { constexpr int t[kLanesBands] = {0, 1, 2, 6, 4, 5}; return t[band]; }
    static constexpr int parts(int band) { constexpr int t[kLanesBands] = {1, 1, 2, 2, 1, 1}; return t[band]; }
#if defined(__HIPCC__)
    using G = GroupDev<8>;
#endif
};
template <>
struct LanesLayout<16> {
    static constexpr int LPO = 16, MAX_PARTS = 4, ALL_ROWS_LANE = 1, WRAP_DPP = 0x11F;       // row_shr:15
    static constexpr int band_of(int lane) { constexpr int t[LPO] = {0, 0, 1, 1, 2, 2, 2, 2, 4, 4, 5, 5, 3, 3, 3, 3}; return t[lane]; }
    static constexpr int first_lane(int band) { constexpr int t[kLanesBands] = {0, 2, 4, 12, 8, 10}; return t[band]; }
    static constexpr int parts(int band) { constexpr int t[kLanesBands] = {2, 2, 4, 4, 2, 2}; return t[band]; }
#if defined(__HIPCC__)
    using G = Lanes16;
#endif
};

// the part of its band a lane holds
template <class L>
constexpr int lanes_part_of(int lane) { return lane - L::first_lane(L::band_of(lane)); }
// The two tables are inverse to each other: a band's lanes are first_lane .. first_lane + parts - 1, an aligned block of
// 2^k lanes (the merge levels pair aligned blocks), and no lane is left over.
template <class L>
constexpr bool lanes_tables_inverse() {
    for (int b = 0; b < kLanesBands; ++b) {
        const int p = L::parts(b), f = L::first_lane(b);
        if (p < 1 || p > L::MAX_PARTS || (p & (p - 1)) != 0 || f % p != 0 || f + p > L::LPO) return false;
        for (int q = 0; q < p; ++q)
            if (L::band_of(f + q) != b) return false;
    }
    for (int l = 0; l < L::LPO; ++l) {
        const int b = L::band_of(l);
        if (b < 0 || b >= kLanesBands || lanes_part_of<L>(l) < 0 || lanes_part_of<L>(l) >= L::parts(b)) return false;
    }
    return lanes_part_of<L>(L::ALL_ROWS_LANE) != 0;
}
template <class L>
constexpr int lanes_parts_total() {
    int total = 0;
    for (int b = 0; b < kLanesBands; ++b) total += L::parts(b);
    return total;
}
static_assert(lanes_tables_inverse<LanesLayout<8>>() && lanes_tables_inverse<LanesLayout<16>>(), "lane -> band and band -> first lane");
static_assert(lanes_parts_total<LanesLayout<8>>() == 8 && lanes_parts_total<LanesLayout<16>>() == 16, "the parts fill the group");

// ---- the index arithmetic of the kernels (plain functions: tests/test_stat_lanes_layout.py runs them on the CPU)
// rows a band may have when a lane holds `cap`
template <class L>
constexpr int lanes_capacity(int band, int cap) { return L::parts(band) * cap; }
// a band of `count` rows is taken (the kernel sends the light curve of one that is not to the retry list)
template <class L>
constexpr bool lanes_band_fits(int band, int count, int cap) { return count <= lanes_capacity<L>(band, cap); }
// merge levels after which the band's sorted sequence is complete
template <class L>
constexpr int lanes_level(int band) {
    int level = 0;
    while ((1 << level) < L::parts(band)) ++level;
    return level;
}
// does a band complete at this level?  (the levels without one are not dumped)
template <class L>
constexpr bool lanes_level_completes(int level) {
    for (int b = 0; b < kLanesBands; ++b)
        if (lanes_level<L>(b) == level) return true;
    return false;
}
// a band of `count` rows over `parts` lanes: rows per part, the rows of part `part`, and whether the pair (last row of
// this part, first row of the next) exists
constexpr int lanes_rows_per_part(int count, int parts) { return (count + parts - 1) / parts; }
constexpr int lanes_part_rows(int count, int h, int part) {
    const int m = count - part * h;
    return (m < 0) ? 0 : ((m > h) ? h : m);
}
constexpr bool lanes_bridge(int count, int h, int part, int parts) { return part + 1 < parts && count > (part + 1) * h; }
// LDS slot of position `pos` of band `band` (hb: rows per part of every band; a column of `stride` doubles per lane):
// lane-major, ascending.  A band of one part never leaves its lane: no rows-per-part is read for it.
constexpr int kLanesOnePart = 1 << 20;
template <class L>
constexpr int lanes_slot(int band, int pos, const int (&hb)[kLanesBands], int stride) {
    int lane = 0, h = kLanesOnePart;
    for (int k = 0; k < kLanesBands; ++k)
        if (band == k) {
            lane = L::first_lane(k);
            if (L::parts(k) > 1) h = hb[k];
        }
    int part = 0;
    for (int q = 1; q < L::MAX_PARTS; ++q) part += (pos >= q * h) ? 1 : 0;
    return (lane + part) * stride + (pos - part * h);
}

}  // namespace lcfe

#if defined(__HIPCC__)
namespace lcfe {

template <int N, int A, int B>
__device__ __forceinline__ void reg_exchange(double (&w)[N]) {
    const double lo = dmin(w[A], w[B]), hi = dmax(w[A], w[B]);
    w[A] = lo;
    w[B] = hi;
}
template <int N, size_t... I>
__device__ __forceinline__ void reg_sort_seq(double (&w)[N], std::index_sequence<I...>) {
    (reg_exchange<N, kOddEvenNet<N>.a[I], kOddEvenNet<N>.b[I]>(w), ...);
}
// ascending sort of N register-resident keys (no NaN among them)
template <int N>
__device__ __forceinline__ void reg_sort(double (&w)[N]) {
    reg_sort_seq<N>(w, std::make_index_sequence<kOddEvenNet<N>.count>{});
}

// half-cleaners of a bitonic sequence held in the registers of one lane: distances D, D/2, .., 1
template <int N, int D>
__device__ __forceinline__ void reg_half_cleaners(double (&w)[N]) {
    if constexpr (D >= 1) {
#pragma unroll
        for (int r = 0; r < N; ++r)
            if ((r & D) == 0) {
                const double lo = dmin(w[r], w[r + D]), hi = dmax(w[r], w[r + D]);
                w[r] = lo;
                w[r + D] = hi;
            }
        reg_half_cleaners<N, D / 2>(w);
    }
}
// half-cleaner between lanes l and l ^ X (same register): the lane with the bit clear keeps the minimum
template <int N, int X>
__device__ __forceinline__ void lane_half_cleaner(double (&w)[N], bool keep_min) {
#pragma unroll
    for (int r = 0; r < N; ++r) {
        const double p = lane_xor_fetch<X>(w[r]);
        w[r] = ((p < w[r]) == keep_min) ? p : w[r];
    }
}
// Merge step over blocks of 2 D lanes: the sequences (lane-major: index = lane * N + register) of the lower and
// the upper D lanes are ascending; afterwards the 2 D lanes hold their union, ascending.  First the element-reversed
// compare (partner lane l ^ (2 D - 1), register N - 1 - r), then half-cleaners at lane distances D / 2 .. 1 and
// register distances N / 2 .. 1.
template <int N, int D>
__device__ __forceinline__ void lane_merge(double (&w)[N], int lane_in_group) {
    {
        const bool keep_min = (lane_in_group & D) == 0;
#pragma unroll
        for (int r = 0; r < N / 2; ++r) {
            const double p1 = lane_xor_fetch<2 * D - 1>(w[N - 1 - r]), p2 = lane_xor_fetch<2 * D - 1>(w[r]);
            w[r] = ((p1 < w[r]) == keep_min) ? p1 : w[r];
            w[N - 1 - r] = ((p2 < w[N - 1 - r]) == keep_min) ? p2 : w[N - 1 - r];
        }
    }
    if constexpr (D >= 8) lane_half_cleaner<N, 4>(w, (lane_in_group & 4) == 0);
    if constexpr (D >= 4) lane_half_cleaner<N, 2>(w, (lane_in_group & 2) == 0);
    if constexpr (D >= 2) lane_half_cleaner<N, 1>(w, (lane_in_group & 1) == 0);
    reg_half_cleaners<N, N / 2>(w);
}

// The lanes kernels index one LDS buffer with computed slots (band position tables, merge dumps, the output rows).
// Release builds use the plain pointer.  A -DLCFE_DEBUG build (make debug; SURVEY.md section 5 "sanitizer" row: the GPU
// AddressSanitizer is not available on this pool) replaces it by a bounds-checked view: an index outside the buffer is
// counted in g_lanes_check[0] (the access is redirected to slot 0 instead of faulting), and the kernel frames the buffer
// with canary words it verifies before it ends (g_lanes_check[1]).  lcfe_debug_lanes_check() reads the counters.
#ifdef LCFE_DEBUG
__device__ unsigned int g_lanes_check[4];      // out-of-range indices, damaged canaries, last bad index, its buffer length
// (branch-free: a bad index is clamped to slot 0 and counted in a per-lane register the kernel flushes when it ends --
//  hundreds of inlined divergent branches around the accesses changed the code the compiler produced for the rest)
struct LanesBuf {
    double* p;
    int n;
    unsigned int* bad;      // per-lane counter (a register of the kernel), [1] = last bad index
    __device__ __forceinline__ double& operator[](int i) const {
        const bool oob = (unsigned int)i >= (unsigned int)n;
        bad[0] += oob ? 1u : 0u;
        bad[1] = oob ? (unsigned int)i : bad[1];
        return p[oob ? 0 : i];
    }
    __device__ __forceinline__ LanesBuf operator+(int k) const { return LanesBuf{p + k, n - k, bad}; }
};
__device__ __forceinline__ LanesBuf lanes_buf(double* p, int n, unsigned int* bad) { return LanesBuf{p, n, bad}; }
// plain pointer to `count` doubles of the view, for the helpers that take one (the range is checked once)
__device__ __forceinline__ double* lanes_raw(const LanesBuf& b, int count) {
    const bool oob = count > b.n || b.n < 0;
    b.bad[0] += oob ? 1u : 0u;
    b.bad[1] = oob ? (unsigned int)count : b.bad[1];
    return b.p;
}
#else
using LanesBuf = double*;
__device__ __forceinline__ LanesBuf lanes_buf(double* p, int, unsigned int*) { return p; }
__device__ __forceinline__ double* lanes_raw(LanesBuf b, int) { return b; }
#endif

template <int CAP>
struct StatLanesLds {
    static constexpr int STRIDE = CAP + 1;       // odd number of doubles: a column per lane without bank conflicts
    double buf[64 * STRIDE];
    double all_rows[8 * 17];                     // the all-rows columns of the eight light curves, stored as they get ready
};

// element `idx` of an ascending sequence dumped lane-major from column `base` on (CAP registers per lane)
template <int CAP>
__device__ __forceinline__ double lanes_seq(LanesBuf buf, int base, int idx) {
    constexpr int SH = (CAP == 16) ? 4 : ((CAP == 32) ? 5 : 6);
    return buf[base + idx + (idx >> SH)];
}

// median, inter-quartile range and MAD of the ascending NaN-free sequence of m >= 1 values at `base`
template <int CAP>
__device__ __forceinline__ void lanes_order_stats(LanesBuf buf, int base, int m, double& med, double& iqr, double& mad) {
    auto S = [&](int i) { return lanes_seq<CAP>(buf, base, i); };
    const int r_lo = (m - 1) / 2, r_hi = m / 2;
    const double v25 = 0.25 * (m - 1), v75 = 0.75 * (m - 1);
    const int r25 = (int)floor(v25), r75 = (int)floor(v75);
    const int r25h = (r25 + 1 < m) ? r25 + 1 : m - 1, r75h = (r75 + 1 < m) ? r75 + 1 : m - 1;
    const double a0 = S(r_lo), a1 = S(r_hi), q0 = S(r25), q1 = S(r25h), q2 = S(r75), q3 = S(r75h);
    med = (r_lo == r_hi) ? a0 : (a0 + a1) / 2.0;
    iqr = (m > 1) ? np_lerp(q2, q3, v75 - r75) - np_lerp(q0, q1, v25 - r25) : 0.0;
    if (!(med - med == 0.0)) { mad = qnan(); return; }
    // stage.hpp::mad_of_sorted with the monotone predicate bisected by this lane alone
    const int h = m / 2, a = m - h, b = h, r = r_lo;
    const int lo = (r + 1 - b > 0) ? r + 1 - b : 0, hi = (a < r + 1) ? a : r + 1;
    int L = lo, H = hi;
    while (L < H) {
        const int c = (L + H) >> 1;
        const bool p = S(h + c) - med < med - S(h - (r + 1 - c));
        L = p ? c + 1 : L;
        H = p ? H : c;
    }
    const int i = L, j = r + 1 - i;
    const double ua = S(h + ((i > 0) ? i - 1 : 0)) - med, la = med - S((j > 0) ? h - j : 0);
    const double ub = S(h + ((i < a) ? i : 0)) - med, lb = med - S((j < b) ? h - 1 - j : 0);
    double v_lo = (i > 0) ? ua : -__builtin_inf();
    v_lo = (j > 0 && la > v_lo) ? la : v_lo;
    double v_hi = (i < a) ? ub : __builtin_inf();
    v_hi = (j < b && lb < v_hi) ? lb : v_hi;
    mad = (r == m / 2) ? v_lo : (v_lo + v_hi) / 2.0;
}

// op over the lanes of one band (`parts` of them, an aligned block): every lane of the band gets the result.  Per
// layout: with one- and two-part bands the fetch sits under a branch, with two- and four-part bands both fetches are
// made and one selected -- one form for both (fetch, then select per doubling) spilled 20 more VGPRs of
// stat_lanes_all_kernel in the 8-lane routes.
template <class L, class V, class Op>
__device__ __forceinline__ V lanes_band(V x, int parts, Op op) {
    if constexpr (L::MAX_PARTS == 2) {
        if (parts == 2) x = op(x, lane_xor_fetch<1>(x));
        return x;
    } else {
        static_assert(L::MAX_PARTS == 4, "one fetch per doubling");
        const V x1 = op(x, lane_xor_fetch<1>(x));
        const V x2 = op(x1, lane_xor_fetch<2>(x1));
        return (parts == 4) ? x2 : x1;
    }
}

// Merge levels LEVEL .. log2(LPO) of the lanes' sorted registers.  A level at which a sequence completes is dumped to
// LDS (lane-major); `reads`: this lane is the first of a band with rows and without NaN, and reads the band's extrema
// and order statistics off the dump of the band's level.  The last dump (the light curve's rows) is left to the caller.
template <class L, int CAP, int LEVEL>
__device__ __forceinline__ void lanes_merge_levels(double (&w)[CAP], LanesBuf buf, int col, int j, bool reads, int parts, int mband,
                                                   double& mn, double& mx, double& med, double& iqr, double& mad) {
    using G = typename L::G;
    constexpr bool last = (1 << LEVEL) == L::LPO;
    if constexpr (LEVEL > 0) lane_merge<CAP, (1 << LEVEL) / 2>(w, j);
    if constexpr (last || lanes_level_completes<L>(LEVEL)) {
#pragma unroll
        for (int i = 0; i < CAP; ++i) buf[col + i] = w[i];
        G::sync();
    }
    if constexpr (!last) {
        if constexpr (lanes_level_completes<L>(LEVEL)) {
            if (reads && parts == (1 << LEVEL)) {
                mn = buf[col];
                mx = lanes_seq<CAP>(buf, col, mband - 1);
                lanes_order_stats<CAP>(buf, col, mband, med, iqr, mad);
            }
            G::sync();
        }
        lanes_merge_levels<L, CAP, LEVEL + 1>(w, buf, col, j, reads, parts, mband, mn, mx, med, iqr, mad);
    }
}

// 64 / LPO light curves (one per LPO-lane group: `obj` < 0 = none; CSR rows [s1, e1)) -> their 123 columns, or list
// `fallback` of `lists` (SetOut and Bins of tickets.hpp: O.row(obj), lists.append(fallback, obj); both are template
// parameters so that this header stands without tickets.hpp for the host-compiled layout tests).  ITERS = rows / LPO a
// light curve of the list may have (band code 256 = no row -- 255 is a code a file may hold).  The rows are loaded in predicated blocks of four trips: one basic block of unconditional loads, a
// persistent batch loop around this function, or exec-masked element loops all made the compiler spill hundreds of
// registers (profiles/r02_stat_instruction_budget.md).
template <int LPO, int CAP, int ITERS, class Out, class Lists>
__device__ __forceinline__ void stat_lanes_batch(const double* gt, const double* gf, const double* ge, const uint8_t* gb, int obj,
                                                 int64_t s1, int64_t e1, LanesBuf buf, LanesBuf all_rows, const Out& O,
                                                 const Lists& lists, int fallback) {
    using L = LanesLayout<LPO>;
    using G = typename L::G;
    constexpr int STRIDE = StatLanesLds<CAP>::STRIDE;
    constexpr int BLK = 4;
    static_assert(ITERS % BLK == 0 && ITERS <= CAP, "rows per lane");
    const int lane = threadIdx.x & 63, j = lane & (LPO - 1), g0 = lane & ~(LPO - 1);
    const int n = (int)(e1 - s1);
    const bool has_obj = obj >= 0;
    bool fit = has_obj && n >= 1 && n <= LPO * ITERS;
    const int nr = fit ? n : 0;
    int nmax = 0;
#pragma unroll
    for (int k = 0; k < 64 / LPO; ++k) { const int v_ = __builtin_amdgcn_readlane(nr, LPO * k); nmax = (v_ > nmax) ? v_ : nmax; }
    constexpr int LOG = (LPO == 8) ? 3 : 4;                 // (shifts: the compiler does not know nmax >= 0)
    const int iters = (nmax + LPO - 1) >> LOG;
    // ---- rows -> registers
    double rt[ITERS], rf[ITERS], rq[ITERS];
    int code[ITERS];
    {
        const double *pt = gt + s1, *pf = gf + s1, *pe = ge + s1;
        const uint8_t* pb = gb + s1;
#pragma unroll
        for (int i0 = 0; i0 < ITERS; i0 += BLK) {
            if (i0 < iters) {
#pragma unroll
                for (int q = 0; q < BLK; ++q) {
                    const int row = (i0 + q) * LPO + j;
                    const bool ok = row < nr;
                    code[i0 + q] = ok ? (int)pb[row] : 256;
                    rt[i0 + q] = ok ? pt[row] : 0.0;
                    rf[i0 + q] = ok ? pf[row] : 0.0;
                    rq[i0 + q] = ok ? pe[row] : 0.0;
                }
            }
        }
    }

    // ---- A: slot of every row inside its band = rows of that band before it (ballots over the LPO rows of a trip)
    int cnt[kLanesBands] = {0, 0, 0, 0, 0, 0};
    bool known = true;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        if ((it & ~(BLK - 1)) < iters) {
            const int b = code[it];
            known = known && (b < 6 || b == 256);
            unsigned int mine = 0;
            int c0 = 0;
#pragma unroll
            for (int k = 0; k < kLanesBands; ++k) {
                const unsigned int mk = (unsigned int)(__ballot(b == k) >> g0) & ((1u << LPO) - 1u);
                if (b == k) { mine = mk; c0 = cnt[k]; }
                cnt[k] += __builtin_popcount(mk);
            }
            const int pos = c0 + __builtin_popcount(mine & ((1u << j) - 1u));
            code[it] = ((b < 6) ? b : 7) | (pos << 8);
        }
    }
    fit = fit && G::all(known);
    // rows per part of every band
    int hb[kLanesBands];
#pragma unroll
    for (int k = 0; k < kLanesBands; ++k) {
        fit = fit && lanes_band_fits<L>(k, cnt[k], CAP);
        hb[k] = lanes_rows_per_part(cnt[k], L::parts(k));
    }
    const int N = fit ? n : 0;
    // this lane's share: band, part, rows = lanes_part_rows / lanes_bridge of the layout's tables (the debug build
    // checks that).  Written out per layout: lookups over the tables (a chain over j == l, one over band == k) moved the
    // register allocation of the 32-rows-per-lane routes -- with the slot expression below 12 -> 68 spilled VGPRs.
    int band, part, parts, mband, h, m;
    bool bridge;                                            // the pair (last row of this part, first row of the next)
    if constexpr (LPO == 8) {
        band = (j == 0) ? 0 : (j == 1) ? 1 : (j <= 3) ? 2 : (j == 4) ? 4 : (j == 5) ? 5 : 3;
        const bool split = (j & 2) != 0, first_ = split && (j & 1) == 0;
        mband = (band == 0) ? cnt[0] : (band == 1) ? cnt[1] : (band == 2) ? cnt[2] : (band == 3) ? cnt[3] : (band == 4) ? cnt[4] : cnt[5];
        h = (band == 2) ? hb[2] : hb[3];
        m = !split ? mband : (first_ ? h : mband - h);
        if (!fit) { m = 0; mband = 0; }
        bridge = first_ && mband > m;
        part = (split && !first_) ? 1 : 0;
        parts = split ? 2 : 1;
    } else {
        band = (j < 2) ? 0 : (j < 4) ? 1 : (j < 8) ? 2 : (j < 10) ? 4 : (j < 12) ? 5 : 3;
        const bool four = (band == 2 || band == 3);
        part = four ? (j & 3) : (j & 1);
        parts = four ? 4 : 2;
        mband = (band == 0) ? cnt[0] : (band == 1) ? cnt[1] : (band == 2) ? cnt[2] : (band == 3) ? cnt[3] : (band == 4) ? cnt[4] : cnt[5];
        h = (band == 0) ? hb[0] : (band == 1) ? hb[1] : (band == 2) ? hb[2] : (band == 3) ? hb[3] : (band == 4) ? hb[4] : hb[5];
        m = mband - part * h;
        m = (m < 0) ? 0 : ((m > h) ? h : m);
        int m_next = mband - (part + 1) * h;
        m_next = (part + 1 < parts && m_next > 0) ? 1 : 0;
        if (!fit) { m = 0; mband = 0; m_next = 0; }
        bridge = m_next != 0;
    }
#ifdef LCFE_DEBUG
    buf.bad[0] += (band != L::band_of(j & (LPO - 1)) || part != lanes_part_of<L>(j & (LPO - 1)) || parts != L::parts(band) ||
                   (fit && (m != lanes_part_rows(mband, lanes_rows_per_part(mband, parts), part) ||
                            bridge != lanes_bridge(mband, lanes_rows_per_part(mband, parts), part, parts))))
                      ? 1u
                      : 0u;
#endif
    const bool first = part == 0;
    const int col = lane * STRIDE;

    // ---- per row: LDS slot (-1: none); the all-rows slope and the order check from the file neighbours (row + 1 = next
    //      lane, or lane 0 of the next trip); the SNR term in place of the error (-0.0 = error bar not positive: the
    //      reference leaves the row out; a term is never negative)
    bool ordered = true, a_snan = false;
    double a_slope = -1.0;
#pragma unroll
    for (int it = 0; it < ITERS; ++it) {
        if ((it & ~(BLK - 1)) < iters) {
            const int b = code[it] & 0xFF, pos = code[it] >> 8;
            // (= g0 * STRIDE + lanes_slot<L>(b, pos, hb, STRIDE); per layout for the same reason, checked by the debug build)
            if constexpr (LPO == 8) {
                const bool second = (b == 2 && pos >= hb[2]) || (b == 3 && pos >= hb[3]);
                const int hs = (b == 2) ? hb[2] : hb[3];
                const int dl = (b == 0) ? 0 : (b == 1) ? 1 : (b == 2) ? 2 : (b == 3) ? 6 : (b == 4) ? 4 : 5;
                code[it] = (b < 6 && fit) ? (g0 + dl + (second ? 1 : 0)) * STRIDE + (second ? pos - hs : pos) : -1;
            } else {
                const int hh = (b == 0) ? hb[0] : (b == 1) ? hb[1] : (b == 2) ? hb[2] : (b == 3) ? hb[3] : (b == 4) ? hb[4] : hb[5];
                const int jb = (b == 0) ? 0 : (b == 1) ? 2 : (b == 2) ? 4 : (b == 3) ? 12 : (b == 4) ? 8 : 10;
                const int p = ((pos >= hh) ? 1 : 0) + ((pos >= 2 * hh) ? 1 : 0) + ((pos >= 3 * hh) ? 1 : 0);
                code[it] = (b < 6 && fit) ? (g0 + jb + p) * STRIDE + (pos - p * hh) : -1;
            }
#ifdef LCFE_DEBUG
            buf.bad[0] += (b < 6 && fit && code[it] != g0 * STRIDE + lanes_slot<L>(b, pos, hb, STRIDE)) ? 1u : 0u;
#endif
            const int row = it * LPO + j;
            const bool has = row + 1 < N;
            const double tn_l = WaveDev::dpp<0x101>(rt[it]), fn_l = WaveDev::dpp<0x101>(rf[it]);        // row_shl:1
            const double tn_w = WaveDev::dpp<L::WRAP_DPP>(rt[(it + 1 < ITERS) ? it + 1 : it]),
                         fn_w = WaveDev::dpp<L::WRAP_DPP>(rf[(it + 1 < ITERS) ? it + 1 : it]);
            const double t1 = (j == LPO - 1) ? tn_w : tn_l, f1 = (j == LPO - 1) ? fn_w : fn_l;
            ordered = ordered && !(has && !(rt[it] <= t1));
            const double dt = t1 - rt[it];
            const double sl = stat_slope(f1 - rf[it], dt);
            const bool valid = has && dt > 0;
            a_snan = a_snan || (valid && is_nan(sl));
            a_slope = (valid && sl > a_slope) ? sl : a_slope;
            rq[it] = (rq[it] > 0) ? fabs(rf[it]) / rq[it] : -0.0;
        }
    }

    // ---- F: fluxes -> lanes (the columns are cleared first: the slots behind a lane's rows read as 0.0 in every phase)
#pragma unroll
    for (int i = 0; i < STRIDE; ++i) buf[col + i] = 0.0;
    G::sync();
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
        if ((it & ~(BLK - 1)) < iters && code[it] >= 0) buf[code[it]] = rf[it];
    G::sync();
    double v[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) v[i] = buf[col + i];
    // (the next lane's first row: read only where `bridge` holds; the wavefront's last lane has no next column)
    const double f_last = buf[col + ((m > 0) ? m - 1 : 0)], f_next = buf[col + ((lane < 63) ? STRIDE : 0)];
    double s;
    bool nanf = false;
    {
        double sa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            sa[i & 3] += v[i];
            nanf = nanf || is_nan(v[i]);
        }
        s = (sa[0] + sa[1]) + (sa[2] + sa[3]);
    }
    G::sync();

    // ---- T: times -> lanes, band slopes against the register-resident fluxes
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
        if ((it & ~(BLK - 1)) < iters && code[it] >= 0) buf[code[it]] = rt[it];
    G::sync();
    double slope = -1.0, tmn, tmx;
    bool snan = false;
    {
        double tc = buf[col];
        tmn = tc;
#pragma unroll
        for (int i = 0; i + 1 < CAP; ++i) {
            const double tn = buf[col + i + 1];
            const double dt = tn - tc;
            const double sl = stat_slope(v[i + 1] - v[i], dt);
            const bool valid = i + 1 < m && dt > 0;
            snan = snan || (valid && is_nan(sl));
            slope = (valid && sl > slope) ? sl : slope;
            tc = tn;
        }
        tmx = buf[col + ((m > 0) ? m - 1 : 0)];
        if (bridge) {
            const double dt = buf[col + STRIDE] - tmx;
            const double sl = stat_slope(f_next - f_last, dt);
            const bool valid = dt > 0;
            snan = snan || (valid && is_nan(sl));
            slope = (valid && sl > slope) ? sl : slope;
        }
    }
    G::sync();

    // ---- Q: SNR terms -> lanes
#pragma unroll
    for (int it = 0; it < ITERS; ++it)
        if ((it & ~(BLK - 1)) < iters && code[it] >= 0) buf[code[it]] = rq[it];
    G::sync();
    double snr;
    int nsnr = m;
    {
        double qa[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            const double qv = buf[col + i];
            qa[i & 3] += qv;
            nsnr -= (int)((unsigned long long)__builtin_bit_cast(long long, qv) >> 63);
        }
        snr = (qa[0] + qa[1]) + (qa[2] + qa[3]);
    }
    G::sync();

    // ---- pass-1 totals: over the light curve, and per band (the lanes of the band combined; a part without rows has no
    //      first or last time)
    const double sA = G::sum(s), snrA = G::sum(snr);
    const int nsnrA = G::sum(nsnr);
    const bool nanA = G::any(nanf);
    const double a_slopeA = G::max(a_slope);
    const bool a_snanA = G::any(a_snan);
    const bool orderedA = G::all(ordered);
    tmn = (m > 0) ? tmn : __builtin_inf();
    tmx = (m > 0) ? tmx : -__builtin_inf();
    const double tmnA = G::min(tmn), tmxA = G::max(tmx);
    auto add = [](auto a, auto b) { return a + b; };
    auto mxo = [](auto a, auto b) { return (b > a) ? b : a; };
    auto mno = [](auto a, auto b) { return (b < a) ? b : a; };
    // (LPO = 8: the fetches of a pass under ONE branch on the split lanes, not one per value -- 1 -> 0 spilled VGPRs in its
    //  routes, which the whole kernel needs to stay at the 25 it had)
    if constexpr (LPO == 8) {
        if (parts == 2) {
            const int p_nan = lane_xor_fetch<1>(nanf ? 1 : 0), p_snan = lane_xor_fetch<1>(snan ? 1 : 0);
            s += lane_xor_fetch<1>(s);
            snr += lane_xor_fetch<1>(snr);
            nsnr += lane_xor_fetch<1>(nsnr);
            nanf = nanf | (p_nan != 0);
            const double p_tmn = lane_xor_fetch<1>(tmn), p_tmx = lane_xor_fetch<1>(tmx), p_slope = lane_xor_fetch<1>(slope);
            tmn = (p_tmn < tmn) ? p_tmn : tmn;
            tmx = (p_tmx > tmx) ? p_tmx : tmx;
            slope = (p_slope > slope) ? p_slope : slope;
            snan = snan | (p_snan != 0);
        }
    } else {
        s = lanes_band<L>(s, parts, add);
        snr = lanes_band<L>(snr, parts, add);
        nsnr = lanes_band<L>(nsnr, parts, add);
        nanf = lanes_band<L>(nanf ? 1 : 0, parts, mxo) != 0;
        snan = lanes_band<L>(snan ? 1 : 0, parts, mxo) != 0;
        slope = lanes_band<L>(slope, parts, mxo);
        tmn = lanes_band<L>(tmn, parts, mno);
        tmx = lanes_band<L>(tmx, parts, mxo);
    }
    const double mean = s / mband, meanA = sA / N;
    LanesBuf oa = all_rows + (g0 >> LOG) * 17;             // the all-rows columns leave the registers as soon as they are known
    if (j == L::ALL_ROWS_LANE) {
        oa[0] = (double)N;
        oa[1] = meanA;
        oa[13] = (N > 1) ? (a_snanA ? qnan() : (a_slopeA < 0 ? 0.0 : a_slopeA)) : 0.0;
        oa[14] = (nsnrA > 0) ? snrA / nsnrA : qnan();
        oa[15] = (N > 1) ? (tmxA - tmnA) : 0.0;
        oa[16] = (N > 1) ? (tmxA - tmnA) / (double)(N - 1) : 0.0;
    }

    // ---- behind the lane's rows the band mean: the centred band passes need no per-element mask (a padded slot adds
    //      exactly 0 and counts as "inside"); the all-rows terms are masked
#pragma unroll
    for (int i = 0; i < CAP; ++i) v[i] = (i < m) ? v[i] : mean;
    // ---- pass 2
    double m2, m2A;
    {
        double a[2] = {0.0, 0.0}, aA[2] = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            const double d = v[i] - mean, dA = (i < m) ? v[i] - meanA : 0.0;
            a[i & 1] += d * d;
            aA[i & 1] += dA * dA;
        }
        m2 = a[0] + a[1];
        m2A = aA[0] + aA[1];
    }
    m2A = G::sum(m2A);
    m2 = lanes_band<L>(m2, parts, add);
    const double sd = (mband > 1) ? sqrt(m2 / mband) : 0.0, sdA = (N > 1) ? sqrt(m2A / N) : 0.0;

    // ---- pass 3 (the lanes of a light curve whose spread is not positive carry garbage that is dropped below)
    double s3, s4, s3A, s4A;
    int c1 = 0, c2 = 0, c1A = 0, c2A = 0;
    {
        const double inv = 1.0 / sd, sd2 = 2.0 * sd, invA = 1.0 / sdA, sdA2 = 2.0 * sdA;
        double a3[2] = {0.0, 0.0}, a4[2] = {0.0, 0.0}, b3[2] = {0.0, 0.0}, b4[2] = {0.0, 0.0};
#pragma unroll
        for (int i = 0; i < CAP; ++i) {
            const double d = v[i] - mean, dA = (i < m) ? v[i] - meanA : 0.0;
            const double zz = d * inv, zA = dA * invA;
            const double z2 = zz * zz, zA2 = zA * zA;
            a3[i & 1] += z2 * zz;
            a4[i & 1] += z2 * z2;
            b3[i & 1] += zA2 * zA;
            b4[i & 1] += zA2 * zA2;
            const double ad = fabs(d), adA = fabs(dA);
            c1 += (ad > sd) ? 1 : 0;
            c2 += (ad > sd2) ? 1 : 0;
            c1A += (adA > sdA) ? 1 : 0;
            c2A += (adA > sdA2) ? 1 : 0;
        }
        s3 = a3[0] + a3[1];
        s4 = a4[0] + a4[1];
        s3A = b3[0] + b3[1];
        s4A = b4[0] + b4[1];
    }
    s3A = G::sum(s3A);
    s4A = G::sum(s4A);
    c1A = G::sum(c1A);
    c2A = G::sum(c2A);
    if constexpr (LPO == 8) {
        if (parts == 2) {
            s3 += lane_xor_fetch<1>(s3);
            s4 += lane_xor_fetch<1>(s4);
            c1 += lane_xor_fetch<1>(c1);
            c2 += lane_xor_fetch<1>(c2);
        }
    } else {
        s3 = lanes_band<L>(s3, parts, add);
        s4 = lanes_band<L>(s4, parts, add);
        c1 = lanes_band<L>(c1, parts, add);
        c2 = lanes_band<L>(c2, parts, add);
    }
    auto finish = [](int cnt_, double sd_, double s3_, double s4_, int c1_, int c2_, double& skew, double& kurt, double& b1, double& b2) {
        skew = 0.0; kurt = 0.0; b1 = 0.0; b2 = 0.0;
        if (sd_ > 0) {
            if (cnt_ > 2) skew = s3_ / cnt_;
            if (cnt_ > 3) kurt = s4_ / cnt_ - 3.0;
            b1 = (double)c1_ / cnt_;
            b2 = (double)c2_ / cnt_;
        } else if (is_nan(sd_)) {
            skew = (cnt_ > 2) ? qnan() : 0.0;
            kurt = (cnt_ > 3) ? qnan() : 0.0;
        }
    };
    double skew, kurt, b1, b2, skewA, kurtA, b1A, b2A;
    finish(mband, sd, s3, s4, c1, c2, skew, kurt, b1, b2);
    finish(N, sdA, s3A, s4A, c1A, c2A, skewA, kurtA, b1A, b2A);
    if (j == L::ALL_ROWS_LANE) {
        oa[2] = sdA;
        oa[6] = skewA;
        oa[7] = kurtA;
        oa[11] = b1A;
        oa[12] = b2A;
    }

    // ---- order statistics and extrema: register sort per lane, then merges across the lanes; a sequence's extrema
    //      and order statistics are read off the LDS dump of the level that completes it
    double w[CAP];
#pragma unroll
    for (int i = 0; i < CAP; ++i) w[i] = (i < m) ? v[i] : __builtin_inf();
    reg_sort<CAP>(w);
    double mn = qnan(), mx = qnan(), med = qnan(), iqr = qnan(), mad = qnan();
    lanes_merge_levels<L, CAP, 0>(w, buf, col, j, first && mband > 0 && !nanf, parts, mband, mn, mx, med, iqr, mad);
    if (j == L::ALL_ROWS_LANE) {
        double mnA = qnan(), mxA = qnan(), medA = qnan(), iqrA = qnan(), madA = qnan();
        if (N > 0 && !nanA) {
            mnA = buf[g0 * STRIDE];
            mxA = lanes_seq<CAP>(buf, g0 * STRIDE, N - 1);
            lanes_order_stats<CAP>(buf, g0 * STRIDE, N, medA, iqrA, madA);
        }
        if (N <= 1) iqrA = 0.0;
        oa[3] = mnA;
        oa[4] = mxA;
        oa[8] = mxA - mnA;
        oa[5] = medA;
        oa[9] = madA;
        oa[10] = iqrA;
    }
    G::sync();
    if (mband <= 1) iqr = 0.0;                               // statistical.py:86: 0 unless the group has two rows

    // ---- the 123 columns of every light curve -> LDS rows -> global
    LanesBuf o = buf + (g0 >> LOG) * 128;
    if (fit && first) {
        double* ob = lanes_raw(o + 17 * band, 17);
        if (mband == 0) stat_empty_group(ob, nullptr);
        else stat_write17(ob, mband, mean, sd, mn, mx, med, skew, kurt, mad, iqr, b1, b2, slope, snan, snr, nsnr, tmn, tmx);
    }
    G::sync();
    if (fit) {
#pragma unroll
        for (int c = j; c < 17; c += LPO) o[102 + c] = oa[c];
    }
    G::sync();
    if (fit && j == 0) stat_cross_band(lanes_raw(o, STAT_NCOL));
    G::sync();
    // rows to global memory, one light curve at a time on the whole wavefront (two 512-byte stores per row)
    const bool done = fit && orderedA;
#pragma unroll
    for (int r = 0; r < 64 / LPO; ++r) {
        const int obj_r = __builtin_amdgcn_readlane(done ? obj : -1, LPO * r);
        if (obj_r >= 0) {
            double* row = O.row(obj_r);
            LanesBuf src = buf + r * 128;
            row[lane] = src[lane];
            if (lane + 64 < STAT_NCOL) row[lane + 64] = src[lane + 64];
        }
    }
    if (!done && has_obj && j == 0) lists.append(fallback, obj);
    G::sync();
}

// One workgroup = one batch (`batch`) of 64 / LPO consecutive list entries; `buf`: 64 x (CAP + 1) doubles of LDS.
template <int LPO, int CAP, int ITERS, class Out, class Lists>
__device__ __forceinline__ void stat_lanes_run(const int64_t* offsets, const double* gt, const double* gf, const double* ge,
                                               const uint8_t* gb, const int* list, int count, int batch, LanesBuf buf, LanesBuf all_rows,
                                               const Out& O, const Lists& lists, int fallback) {
    const int g = (threadIdx.x & 63) / LPO;
    const int64_t base = (int64_t)batch * (64 / LPO);
    int obj = -1;
    int64_t s1 = 0, e1 = 0;
    if (base + g < count) {
        obj = list[base + g];
        s1 = offsets[obj];
        e1 = offsets[obj + 1];
    }
    stat_lanes_batch<LPO, CAP, ITERS>(gt, gf, ge, gb, obj, s1, e1, buf, all_rows, O, lists, fallback);
}

}  // namespace lcfe
#endif
