// gp_tier_table.hpp -- THE table of the 2-D GP's tiers: one row per tier, and the only place a tier's numbers are written.
// Plain C++ (no device code, no other header of the project): gp.hpp, gp_tiers.hpp, workspace.hpp, the device probe and
// the host simulation all read it.  To move a tier (matrix to LDS or to global scratch, another workgroup size, another
// grid, another row capacity) edit its row and nothing else; tests/test_gp_tier_table_cpu.py then names the Python tables
// of the tests that have to follow.
#pragma once
#include <cstddef>
#include <cstdint>

namespace lcfe {

// doubles of the tile-packed lower triangle of an np-row matrix (gp.hpp: 16 x 16 tiles of 256 doubles)
constexpr int gp_store_doubles(int np) { return ((np + 15) / 16) * ((np + 15) / 16 + 1) / 2 * 256; }

// X(id, NP, GLOBAL_K, THREADS, WAVES, FUSE, COMPACT, SLABS)
//   NP        row capacity: valid points + the augmented residual row.  The tier takes light curves of up to NP - 1 rows
//             (its cap) and of more rows than the tier before it (tier 0: from the 10 rows gp_object asks for)
//   GLOBAL_K  Gram matrix in a per-workgroup slab of global scratch (L2-resident), not in LDS: the LDS then holds only the
//             pivot panels and two to four workgroups share a CU
//   THREADS   of the workgroup
//   WAVES     waves per SIMD the register allocation leaves room for (__launch_bounds__): tiers that fit two or more
//             workgroups per CU halve their register budget (the L-BFGS-B driver spills a little, the sweep does not)
//   FUSE      the sweep takes two pivot tiles per pass: global-scratch tiers whose second pivot panel fits LDS
//   COMPACT   row-update loops over compacted trip lists, only the tiles a pass stores (gp_sweep_inverse), where that
//             was measured to win; needs the pivot look-ahead and an LDS working set
//   SLABS     Gram-matrix slabs of the tier in the workspace = most workgroups of its grid (GLOBAL_K tiers; a tier in LDS
//             keeps the figure it would get)
// Measured (125,000 objects): with their matrix in global scratch the 112- and 160-row tiers both gain 8-9 % serialised;
// with the fit kernels running beside the GP (the default schedule) the 112-row tier gains 1.5 % end to end and the
// 160-row tier LOSES 5 % -- so only the former.
#define LCFE_GP_TIERS(X)                          \
    X(0, 64, false, 256, 3, false, true, 0)       \
    X(1, 112, true, 256, 4, true, false, 1024)    \
    X(2, 160, false, 512, 2, false, true, 512)    \
    X(3, 240, true, 512, 4, true, false, 512)     \
    X(4, 512, true, 512, 2, true, true, 256)      \
    X(5, 768, true, 1024, 4, false, false, 256)

struct GpTierRow {
    int id, np;
    bool global_k;
    int threads, waves;
    bool fuse, compact;
    int slabs;
};
#define LCFE_GP_TIER_ROW(id, NP, GK, T, WV, FUSE, COMPACT, SLABS) {id, NP, GK, T, WV, FUSE, COMPACT, SLABS},
constexpr GpTierRow kGpTierTable[] = {LCFE_GP_TIERS(LCFE_GP_TIER_ROW)};
#undef LCFE_GP_TIER_ROW
constexpr int kGpNumTiers = (int)(sizeof(kGpTierTable) / sizeof(kGpTierTable[0]));
constexpr int kGpMinRows = 10;         // gp_object fits no light curve of fewer valid points

constexpr int gp_tier_cap(int ti) { return kGpTierTable[ti].np - 1; }
constexpr int gp_tier_first(int ti) { return (ti == 0) ? kGpMinRows : kGpTierTable[ti - 1].np; }
constexpr int kGpLastCap = gp_tier_cap(kGpNumTiers - 1);   // longer light curves: the long-object tier (gp_tiers.hpp)
// bytes of a tier's region of the workspace: one slab per workgroup of its largest grid
constexpr size_t gp_tier_slab_bytes(int ti) {
    return kGpTierTable[ti].global_k ? (size_t)kGpTierTable[ti].slabs * gp_store_doubles(kGpTierTable[ti].np) * 8 : 0;
}
// the row of the tier of capacity NP (id -1: no tier has this capacity; GpTier of gp_tiers.hpp refuses it)
constexpr GpTierRow gp_tier_row(int np) {
    for (int ti = 0; ti < kGpNumTiers; ++ti)
        if (kGpTierTable[ti].np == np) return kGpTierTable[ti];
    return GpTierRow{-1, np, false, 0, 0, false, false, 0};
}

// the tier of a light curve of n rows (kGpNumTiers: beyond the last cap), and a tier's cap for a tier id that is only
// known at run time: chains of comparisons against constants, for the device as well as the host
constexpr int gp_bin_of(int64_t n) {
#define LCFE_GP_TIER_BIN(id, NP, ...) (n <= NP - 1) ? id:
    return LCFE_GP_TIERS(LCFE_GP_TIER_BIN) kGpNumTiers;
#undef LCFE_GP_TIER_BIN
}
constexpr int gp_cap_of(int tier) {
#define LCFE_GP_TIER_CAP(id, NP, ...) (tier == id && id < kGpNumTiers - 1) ? NP - 1:
    return LCFE_GP_TIERS(LCFE_GP_TIER_CAP) kGpLastCap;      // (the last tier's cap for every id beyond it)
#undef LCFE_GP_TIER_CAP
}
// the last tier a launch sequence needs: the first whose cap reaches max_len
constexpr int gp_last_tier(int64_t max_len) {
    const int bin = gp_bin_of(max_len);
    return (bin < kGpNumTiers) ? bin : kGpNumTiers - 1;
}

#define LCFE_GP_TIER_CHECK(I, NP, GK, T, WV, FUSE, COMPACT, SLABS)                                                               \
    static_assert(kGpTierTable[I].id == I && gp_tier_first(I) < NP, "tiers in the order of their ids and of their capacities"); \
    static_assert(T % 64 == 0 && (!FUSE || GK) && (!GK || SLABS > 0), "a fused sweep and slabs go with a matrix in global scratch"); \
    static_assert(gp_tier_slab_bytes(I) % 256 == 0, "slab regions are multiples of the workspace's 256-byte rounding");
LCFE_GP_TIERS(LCFE_GP_TIER_CHECK)
#undef LCFE_GP_TIER_CHECK

}  // namespace lcfe
