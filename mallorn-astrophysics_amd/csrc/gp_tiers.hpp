// gp_tiers.hpp -- what the 2-D GP's kernels build from a row of the tier table (gp_tier_table.hpp, the only place a tier's
// numbers are written): launch bounds by NP, the working-set type, the matrix pointer type and the call of gp_eval -- one
// declaration of "how a tier evaluates" -- and the long-object tier, which is no row of the table.  Shared by the tier
// kernels of lcfe.hip and by the device probe of the objective (tests/devprobe/gp_probe.hip), so that the probe evaluates
// as a tier does by construction.  To move a tier, edit its row of the table; nothing here or in the kernels changes.
#pragma once
#include <type_traits>

#include "gp.hpp"

namespace lcfe {

// the long-object tier of the 2-D GP: light curves of more than kGpLastCap rows, up to kGpLongNP - 1 valid points; Gram
// matrix AND working set (panels, point arrays, optimiser state) in per-workgroup slabs of global scratch
constexpr int kGpLongNP = 2048, kGpLongThreads = 1024, kGpLongGrid = 8;

// launch bounds of gp_kernel<NP, GLOBAL_K> / gp_long_kernel
template <int NP> struct gp_threads { static constexpr int T = (NP == kGpLongNP) ? kGpLongThreads : gp_tier_row(NP).threads; };
template <int NP> struct gp_waves { static constexpr int N = gp_tier_row(NP).waves; };

// how a workgroup of NP-row capacity evaluates the objective: policy W, working set Set, matrix K addressed as a KPtr
// (USER: the policy's tag -- the grid kernels evaluate on a policy of their own, BlockDev of wave.hpp)
template <int NP, class SET, class KPTR, int USER = 0>
struct GpEvalAs {
    using W = BlockDev<gp_threads<NP>::T, USER>;
    using Set = SET;
    using KPtr = KPTR;
    static __device__ __forceinline__ void eval(Set& S, double* K, const double* x, int n, double& f, double* g, bool need) {
        gp_eval<W, NP, KPtr>(x, n, S, (KPtr)K, f, g, need);
    }
};
// a tier of the table: working set in LDS, matrix in LDS (kLdsDoubles of the kernel's own) or in the workgroup's slab
template <int NP, bool GLOBAL_K, int USER = 0>
struct GpTier : GpEvalAs<NP, GpLds<NP, gp_threads<NP>::T / 64, gp_tier_row(NP).fuse, true, true, gp_tier_row(NP).compact>,
                         std::conditional_t<GLOBAL_K, global_double*, lds_double*>, USER> {
    static constexpr GpTierRow kRow = gp_tier_row(NP);
    static_assert(kRow.id >= 0 && kRow.global_k == GLOBAL_K, "gp_kernel<NP, GLOBAL_K> is a row of LCFE_GP_TIERS");
    static constexpr int kLdsDoubles = GLOBAL_K ? 1 : gp_store_doubles(NP);
    // (called where eval is called, with the kernel's own __shared__ array: gp_eval of an LDS tier then sees a constant)
    static __device__ __forceinline__ double* matrix(double* lds, double* slab) { return GLOBAL_K ? slab : lds; }
};
// (the long tier has no pivot look-ahead: its staging tile is handed over between lanes of one wavefront under wave-level
//  fences, which the tiers rely on for LDS only)
template <int USER>
struct GpLongTierOf : GpEvalAs<kGpLongNP, GpLds<kGpLongNP, kGpLongThreads / 64, false, false, false>, global_double*, USER> {
    // slabs of the workspace: kGpLongGrid Gram matrices, then kGpLongGrid working sets
    static constexpr size_t kSetBytes = (sizeof(typename GpLongTierOf::Set) + 255) & ~(size_t)255;
    static constexpr size_t kBytes = (size_t)kGpLongGrid * ((size_t)gp_store_doubles(kGpLongNP) * 8 + kSetBytes);
};
using GpLongTier = GpLongTierOf<0>;
constexpr int kGpGridUser = 1;         // the policy tag of gp_grid_kernel / gp_grid_long_kernel

}  // namespace lcfe
