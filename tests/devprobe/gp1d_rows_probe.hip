// gp1d_rows_probe.hip -- device probe of the per-band GP's row builder, Gp1dRows::build of csrc/gp1d_rows.hpp.
//
// Test infrastructure (tests/test_gpu_gp1d_rows.py), never loaded by the product path.  ONE workgroup of 256 threads, the
// thread count of gp1d_kernel and gp1d_long_kernel, takes the slices of a case list one after the other through the same
// LDS object, as a persistent product kernel takes its light curves: what an earlier slice left in LDS is still there when
// the next one is built.  Per slice it copies out boff[5], nall[4], the ordered flag and rows[0 .. boff[4]).
//
// Conventions of probe.hip: host pointers in, sizes checked on the host, one launch, guard bytes behind every output; the
// probe's own loop runs over the case list only.
#include "gp1d_rows.hpp"

#include "call.hpp"

using namespace lcfe;

namespace {

constexpr int kRowsThreads = 256;
constexpr int kRowsMaxCases = 256;         // slices of one call
constexpr int kRowsHead = 10;              // ints per slice: boff[5], nall[4], ordered

struct RowsProbeArgs {
    const int* off;                        // [ncase + 1] slice c = rows off[c] .. off[c + 1) of t, f, e, b
    const double *t, *f, *e;
    const unsigned char* b;
    int ncase;
    int* head;                             // [ncase][kRowsHead]
    unsigned short* rows;                  // [ncase][ROWCAP], slots boff[4] .. ROWCAP left as they are
};

template <int ROWCAP, int SORTCAP>
__global__ __launch_bounds__(kRowsThreads) void k_gp1d_rows(RowsProbeArgs a) {
    __shared__ Gp1dRows<kRowsThreads, ROWCAP, SORTCAP> R;
    const int lane = threadIdx.x;
    for (int c = 0; c < a.ncase; ++c) {
        const int s = a.off[c], n = a.off[c + 1] - s;
        const bool ordered = R.build(a.t + s, a.f + s, a.e + s, a.b + s, n);
        int* h = a.head + (size_t)c * kRowsHead;
        if (lane < 5) h[lane] = R.boff[lane];
        else if (lane < 9) h[lane] = R.nall[lane - 5];
        else if (lane == 9) h[lane] = ordered ? 1 : 0;
        for (int k = lane; k < R.boff[4]; k += kRowsThreads) a.rows[(size_t)c * ROWCAP + k] = R.rows[k];
        __syncthreads();
    }
}

// shape ids of the ABI: {ROWCAP, SORTCAP}
#define GP1D_ROWS_SHAPES(X) X(0, 768, 768) X(1, 320, 64)

bool rows_shape(int shape, int& rowcap, int& sortcap) {
    switch (shape) {
#define X(id, RC, SC) case id: rowcap = RC; sortcap = SC; return true;
        GP1D_ROWS_SHAPES(X)
#undef X
    }
    return false;
}

}  // namespace

extern "C" {

// o[4]: threads of the workgroup, ROWCAP, SORTCAP, most slices of one call
int devprobe_gp1d_rows_info(int shape, int* o) {
    int rowcap, sortcap;
    if (!rows_shape(shape, rowcap, sortcap)) return kBadShape;
    o[0] = kRowsThreads; o[1] = rowcap; o[2] = sortcap; o[3] = kRowsMaxCases;
    return 0;
}

// One workgroup builds the rows of slice 0, 1, .. ncase - 1 in this order.  head: [ncase][10], rows: [ncase][ROWCAP].
int devprobe_gp1d_rows(int shape, int ncase, const int* off, const double* t, const double* f, const double* e, const unsigned char* b,
                       int* head, unsigned short* rows) {
    int rowcap, sortcap;
    if (!rows_shape(shape, rowcap, sortcap)) return kBadShape;
    if (ncase < 1 || ncase > kRowsMaxCases || off[0] != 0) return kBadSize;
    for (int c = 0; c < ncase; ++c)
        if (off[c + 1] < off[c] || off[c + 1] - off[c] > rowcap) return kBadSize;
    const size_t total = (size_t)off[ncase];
    Call c;
    RowsProbeArgs a;
    a.off = c.in(off, (size_t)ncase + 1);
    a.t = c.in(t, total);
    a.f = c.in(f, total);
    a.e = c.in(e, total);
    a.b = c.in(b, total);
    a.ncase = ncase;
    a.head = c.out(head, (size_t)ncase * kRowsHead);
    a.rows = c.out(rows, (size_t)ncase * rowcap);
    if (c.ok()) {
        switch (shape) {
#define X(id, RC, SC) case id: k_gp1d_rows<RC, SC><<<1, kRowsThreads>>>(a); break;
            GP1D_ROWS_SHAPES(X)
#undef X
        }
    }
    return c.finish();
}

}  // extern "C"
