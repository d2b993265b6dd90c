// gp1d_tiers.hpp -- the tiers of the per-band GP (gp1d.hpp): workgroup size, the two LDS layouts of gp1d_kernel, the
// global-scratch matrix of a long band, the long-object tier's working set, the slab sizes, and the table of the
// gp1d_kernel instantiations.  Shared by the kernels and the launcher of lcfe.hip and by the device probe of the
// objective (tests/devprobe/gp1d_probe.hip), so that the probe instantiates gp1d_eval exactly as a tier does.
#pragma once
#include "gp1d.hpp"
#include "gp_tiers.hpp"

namespace lcfe {

constexpr int kGp1dLongNP = 768;        // rows of the global-scratch matrix of a long band (160..767 valid points)
constexpr int kGp1dLongGrid = 256;
constexpr size_t kGp1dLongBytes = (size_t)kGp1dLongGrid * gp_store_doubles(kGp1dLongNP) * 8;
constexpr int kGp1dThreads = 256;       // measured: 64 threads 10.1 s, 128: 7.2 s, 256: 6.8 s per 125 k objects
// ---- per-band 1-D GP (gp1d.hpp): one light curve per workgroup of kGp1dThreads threads, its bands g, r, i, z one after
// the other; the band's rows are an index list into the CSR slice (time order: file order when the rows
// are sorted, a rank sort otherwise); NP - 1 = most valid points of a band, ROWCAP = most rows of the object
// Bands of at most WNP - 1 valid points (the common case) are fitted by the four wavefronts of the workgroup
// side by side, each on a WNP-row matrix of its own with wave-level fences only; otherwise the bands run one
// after the other on the whole workgroup with the NP-row matrix.  Both layouts share one LDS buffer.
template <int WNP>
struct Gp1dWaveLds {
    Gp1dLds<WNP, 1> S;
    double K[gp_store_doubles(WNP)];
};
template <int NP, int NW>
struct Gp1dBlockLds {
    Gp1dLds<NP, NW> S;
    double K[gp_store_doubles(NP)];
};
// bytes of that buffer: the NP-row layout of the whole workgroup or the four WNP-row slices of its wavefronts (a workgroup
// of another size than kGp1dThreads has no wave path)
template <int NP, int T, int WNP>
constexpr size_t gp1d_lds_bytes() {
    constexpr size_t kBlockBytes = sizeof(Gp1dBlockLds<NP, T / 64>), kWaveBytes = (T == 256) ? 4 * sizeof(Gp1dWaveLds<WNP>) : 0;
    return (kBlockBytes > kWaveBytes) ? kBlockBytes : kWaveBytes;
}

// the gp1d_kernel<NP, ROWCAP, kGp1dThreads, WNP, MW> instantiations, by tier of the launcher (tiers 3..5 share the last):
// X(tier, NP, ROWCAP, WNP, MW); MW = waves per SIMD the register allocation leaves room for.  ROWCAP > NP: the tier fits
// bands of NP .. kGp1dLongNP - 1 valid points on the global-scratch matrix.
#define LCFE_GP1D_KERNEL_TIERS(X) X(0, 64, 64, 32, 3) X(1, 112, 112, 32, 2) X(2, 160, 160, 64, 1) X(3, 160, 768, 64, 1)
constexpr int kGp1dKernelTiers = 4;

// ---- the long-object tier of the per-band GP: light curves of more than 767 rows (GP bin 6), up to kLongCap rows, each band
// up to kGp1dLongTierNP - 1 valid points -- the 2-D GP's limits.  One light curve per workgroup of kGp1dThreads threads, its
// bands one after the other on the whole workgroup, persistent over bin 6 through one ticket counter.  The Gram matrix
// (gp_store_doubles(2048) doubles, 16.9 MB) AND the working set (Gp1dLds<2048, 4> in global scratch, 366 KB) sit in a
// per-workgroup slab; LDS holds the row lists only: 32 KiB of valid row indices partitioned by band + 4 KiB for the rank
// sort of one band + < 1 KiB of counters = 37 KiB of the 160 KiB.
// Grid: 8 workgroups (the 2-D GP's long tier has 8 too): 8 slabs are 138 MB of workspace, 16 would be 276 MB for a tier
// that sees a handful of light curves per batch.  Tickets are served in file order: ordering them longest first would need
// another n_obj-entry index list in every workspace (the one bin-6 list is read by the 2-D GP's long kernel at the same time).
constexpr int kGp1dLongTierNP = kGpLongNP;
constexpr int kGp1dLongTierGrid = 8;
using Gp1dLongTierWs = Gp1dLds<kGp1dLongTierNP, kGp1dThreads / 64, false>;
constexpr size_t kGp1dLongTierSBytes = (sizeof(Gp1dLongTierWs) + 255) & ~(size_t)255;
constexpr size_t kGp1dLongTierBytes = (size_t)kGp1dLongTierGrid * ((size_t)gp_store_doubles(kGp1dLongTierNP) * 8 + kGp1dLongTierSBytes);

}  // namespace lcfe
