// tickets.hpp -- what every persistent kernel of lcfe.hip stands on: how an index list is named and appended to, how a
// workgroup takes its next ticket, how the light curve behind a ticket is fetched, and where its columns and status words
// go.
#pragma once
#include "wave.hpp"
#include "workspace.hpp"

namespace lcfe {

struct BatchView {
    const int64_t* offsets;
    const double* t;
    const double* f;
    const double* e;
    const uint8_t* b;
    const double* z;
    int64_t n_obj;
    // rows [s, s + n) of light curve i; its redshift for the sets that read one (NaN where the caller passed none)
    LCFE_FN ObjIn object(int64_t i, int64_t s, int64_t n, bool with_z) const {
        return {t + s, f + s, e + s, b + s, (int)n, (with_z && z) ? z[i] : qnan()};
    }
};

// Where one set's columns and status words go: row i of the caller's matrices, from the set's first column and word on.
// Passed to the kernels by value, at the offsets the six loose arguments had.  Device functions that are inlined into one
// kernel (the fit loops, the lanes routes) take it by const reference; nan_fill_bins, which many kernels share, takes it by
// value (see there).
struct SetOut {
    double* out;
    int ld, col0;
    int32_t* status;                   // nullptr: the caller takes no status words
    int st_ld, st0;
    LCFE_FN double* row(int64_t i) const { return out + i * (int64_t)ld + col0; }
    // (a set without status words asks `nst ? O.st(i) : nullptr`: st0 is then the next set's first word)
    LCFE_FN int32_t* st(int64_t i) const { return status ? status + i * (int64_t)st_ld + st0 : nullptr; }
    // "not available": NaN in the ncol columns, -100 in the nst status words, on every lane of policy W
    template <class W>
    LCFE_FN void unavailable(int64_t i, int ncol, int nst) const {
        fill_row_nan<W>(row(i), ncol);
        if (status && nst) {
            int32_t* s = st(i);
            for (int k = W::lane(); k < nst; k += W::LANES) s[k] = -100;
        }
    }
    // (host side: launch_stat's view for the general kernel of a set that has no status words)
    SetOut without_status() const { return {out, ld, col0, nullptr, 0, 0}; }
};

// The index lists (ids, count slots and the region behind them: workspace.hpp).  `k` is the same in every lane.
struct Bins {
    int* lists;                        // [kNumLists][n_obj]: set tiers, GP tiers, statistics fallback
    int* counts;                       // [kNumLists]
    int64_t stride;                    // n_obj
#if defined(__HIPCC__)
    __device__ __forceinline__ int* list(int k) const { return lists + (int64_t)k * stride; }
    __device__ __forceinline__ int count(int k) const { return uniform_int(counts[k]); }
    // `n` entries at the end of list k for the caller to fill: the position of the first
    __device__ __forceinline__ int reserve(int k, int n) const { return atomicAdd(&counts[k], n); }
    // One thread appends light curve i.  A list has n_obj entries and takes a light curve at most once per call, so the
    // guard never fires: a caller's mistake would lose an entry (the count then exceeds n_obj) instead of writing behind the list.
    __device__ __forceinline__ void append(int k, int i) const {
        const int slot = reserve(k, 1);
        if (slot < stride) list(k)[slot] = i;
    }
#endif
};

#if defined(__HIPCC__)
// The next ticket of a counter (zeroed once per call) for the whole workgroup: thread 0 draws it, `slot` (a word of LDS
// nothing else touches) and two barriers hand it to every thread.
// THE RULE: what is uniform by construction is made uniform for the compiler before it steers control flow.  A ticket,
// the list entry behind it and that light curve's CSR offsets are the same in every lane, but the compiler sees vector
// loads: a `continue` on a length loaded that way once became an inner loop that re-read the same ticket for ever.  So
// the ticket passes through readfirstlane, and so does what take_object and TicketChunk::object return.
__device__ __forceinline__ int64_t block_ticket(unsigned long long* ticket, long long& slot) {
    if (threadIdx.x == 0) slot = (long long)atomicAdd(ticket, 1ull);
    __syncthreads();
    const long long t = slot;
    __syncthreads();
    return uniform_i64(t);
}

// List entries per ticket: `chunk`, fewer in a sparsely filled list so that every workgroup gets `share` tickets, at least `least`.
__device__ __forceinline__ int ticket_chunk(int count, int chunk, int share, int least) {
    const int per_wave = count / (share * (int)gridDim.x);
    return (per_wave < least) ? least : ((per_wave < chunk) ? per_wave : chunk);
}

// The light curve behind a list entry: index, first CSR row, rows.
struct ListObject { int64_t i, s, n; };
__device__ __forceinline__ ListObject take_object(const BatchView& B, const int* list, int64_t pos) {
    const int64_t i = uniform_int(list[pos]);
    const int64_t s = uniform_i64(B.offsets[i]);
    return {i, s, uniform_i64(B.offsets[i + 1]) - s};
}

// The nk <= 64 entries from `base` on of a ticket of several (workgroups of one wavefront): lane k loads entry k, all
// loads in flight at once; object(k) reads it back from that lane's registers.
struct TicketChunk {
    int obj, n;
    long long s;
    __device__ __forceinline__ void load(const int* list, int64_t base, int nk, const BatchView& B) {
        obj = 0, n = 0, s = 0;
        if ((int)threadIdx.x < nk) {
            obj = list[base + threadIdx.x];
            s = B.offsets[obj];
            n = (int)(B.offsets[obj + 1] - s);
        }
    }
    __device__ __forceinline__ ListObject object(int k) const {
        using W = WaveDev;
        return {W::rdlane(obj, k), ((int64_t)W::rdlane((int)(s >> 32), k) << 32) | (unsigned int)W::rdlane((int)s, k), W::rdlane(n, k)};
    }
};
#endif

}  // namespace lcfe
