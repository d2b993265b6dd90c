// gp1d_rows.hpp -- the band rows of one light curve for the per-band GP (gp1d.hpp): the VALID rows (flux and error not
// NaN, error > 0) of the bands g, r, i, z of a CSR slice as one index list partitioned by band, each part in time order,
// built by one workgroup of T threads.  Device only: gp1d_kernel and gp1d_long_kernel of lcfe.hip and the device probe
// (tests/devprobe/gp1d_rows_probe.hip) share it; the host simulation stages its bands through stage_object instead.
//
// Time order is file order when the whole slice is sorted by time (t[k] <= t[k + 1] for every k), and otherwise a stable
// rank sort of each band by (time, position), as the reference's ``sort_values``: equal times keep their file order and a
// NaN time sorts last (NaN times among themselves in file order), so the ranks are a permutation whatever the input.  A
// NaN time makes the slice unordered, so it always takes the sort.
#pragma once
#include "wave.hpp"

namespace lcfe {

// ROWCAP: entries of `rows` (the slice has at most ROWCAP rows); SORTCAP: entries of the rank sort's one-band scratch.  A
// band of more than SORTCAP valid rows stays in file order: the caller's fit does not take it either.
template <int T, int ROWCAP, int SORTCAP>
struct Gp1dRows {
    static_assert(T % 64 == 0 && ROWCAP <= 65536 && SORTCAP <= ROWCAP, "row indices are 16 bits wide");
    unsigned short rows[ROWCAP];           // band j: rows[boff[j] .. boff[j + 1])
    unsigned short sorted[SORTCAP];
    int boff[5];                           // running count of VALID rows
    int nall[4];                           // ALL rows of the band (the cross-band columns take a band with >= 5 rows)
    int wcnt[T / 64][4];

    // Every thread of the workgroup calls it; rows, boff and nall are complete behind its last barrier.  Returns whether
    // the slice was in time order (the same value in every thread).
    // Not inlined: the kernels that call it sit at their register limit, and it shares no live state with the fits.
    __device__ __noinline__ bool build(const double* t, const double* f, const double* e, const uint8_t* bb, int n) {
        using W = BlockDev<T>;
#if defined(__HIP_DEVICE_COMPILE__)
        __builtin_assume(__builtin_amdgcn_is_shared((const void*)this));   // ds_read / ds_write instead of FLAT operations
#endif
        auto valid = [&](int k) { return !is_nan(f[k]) && !is_nan(e[k]) && e[k] > 0; };
        int cnt[4] = {0, 0, 0, 0}, nv[4] = {0, 0, 0, 0};
        for (int k = threadIdx.x; k < n; k += T) {
            const int band = bb[k];
            if (band < 1 || band > 4) continue;
            ++cnt[band - 1];
            if (valid(k)) ++nv[band - 1];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) { cnt[j] = W::sum(cnt[j]); nv[j] = W::sum(nv[j]); }
        if (threadIdx.x == 0) {
            boff[0] = 0;
            for (int j = 0; j < 4; ++j) { boff[j + 1] = boff[j] + nv[j]; nall[j] = cnt[j]; }
        }
        __syncthreads();
        // stable partition of the valid rows by band: ballot ranks inside a wavefront, wave totals through LDS, running
        // totals per chunk of T rows (one pass over the band bytes, O(n) per object)
        int run[4] = {0, 0, 0, 0};
        for (int base = 0; base < n; base += T) {
            const int k = base + (int)threadIdx.x;
            const int band = (k < n && valid(k)) ? (int)bb[k] : 0;
            int rank = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const unsigned long long mk = __ballot(band == j + 1);
                if (band == j + 1) rank = WaveDev::prefix(mk);
                if ((threadIdx.x & 63) == 0) wcnt[threadIdx.x >> 6][j] = popcll(mk);
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                int before = 0, total = 0;
                for (int wv = 0; wv < T / 64; ++wv) { const int c = wcnt[wv][j]; total += c; before += (wv < (int)(threadIdx.x >> 6)) ? c : 0; }
                if (band == j + 1) rows[boff[j] + run[j] + before + rank] = (unsigned short)k;
                run[j] += total;
            }
            __syncthreads();
        }
        bool ordered = true;
        for (int k = threadIdx.x; k + 1 < n; k += T) ordered = ordered && (t[k] <= t[k + 1]);
        ordered = W::all(ordered);
        if (!ordered) {
            // at most SORTCAP^2 / T comparisons per thread and band
            for (int j = 0; j < 4; ++j) {
                const int b0 = boff[j], m = boff[j + 1] - b0;
                if (m > SORTCAP) continue;
                for (int k = threadIdx.x; k < m; k += T) {
                    const double tk = t[rows[b0 + k]];
                    const bool nk = is_nan(tk);
                    int r = 0;
                    for (int q = 0; q < m; ++q) {
                        const double tq = t[rows[b0 + q]];
                        const bool nq = is_nan(tq);
                        const bool lt = (nq == nk) ? (nk ? q < k : (tq < tk || (tq == tk && q < k))) : nk;
                        r += lt ? 1 : 0;
                    }
                    sorted[r] = rows[b0 + k];
                }
                __syncthreads();
                for (int k = threadIdx.x; k < m; k += T) rows[b0 + k] = sorted[k];
                __syncthreads();
            }
        }
        return ordered;
    }
};

}  // namespace lcfe
