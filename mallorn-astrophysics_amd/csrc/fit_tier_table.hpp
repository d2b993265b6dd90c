// fit_tier_table.hpp -- THE table of the band-length tiers of the fit-by-fit kernels (Bazin and the decline fits): one row
// per tier, and the only place a tier's numbers are written.  Plain C++ (no device code, no other header of the project):
// workspace.hpp, lcfe.hip and the host simulation all read it.  To move a tier (another row capacity, another group width,
// fewer groups per wave, another register budget) edit its row and nothing else; to add one, add its row and keep the ids
// in order: the count and ticket slots, the lists, the partition kernels' binning, the kernels' LDS regions and the launch
// loops follow.  tests/test_fit_tier_table_cpu.py then names the Python restatements of the tests that have to follow.
#pragma once

namespace lcfe {

// X(id, BCAP, LANES, GROUPS, WAVES_BAZIN, WAVES_DECLINE, KERNEL)
//   BCAP           rows of one band: the tier's list takes the fits of bands of up to BCAP rows (for the decline fits:
//                  post-peak rows) and of more rows than the tier before it
//   LANES          lanes of the group that runs one fit (wave.hpp: GroupDev<LANES>)
//   GROUPS         lane groups of a wavefront that take fits, each with an LDS region of its own: all of them while the
//                  regions fit next to each other, six of eight in the 256-row tier
//   WAVES_BAZIN    waves per SIMD the register allocation of the tier's Bazin kernel leaves room for (__launch_bounds__)
//   WAVES_DECLINE  ... of its decline-fit kernels
//   KERNEL         the tier has kernels of its own.  The one tier without is drained by the kernels of the next tier (its
//                  host), which hold its regions in the same LDS: a launch of its own behind the others would add its
//                  longest fit to the end of the fit stream
#define LCFE_FIT_TIERS(X)          \
    X(0, 16, 4, 16, 0, 0, false)   \
    X(1, 32, 8, 8, 2, 2, true)     \
    X(2, 64, 8, 8, 1, 2, true)     \
    X(3, 128, 8, 8, 1, 1, true)    \
    X(4, 256, 8, 6, 1, 1, true)

struct FitTierRow {
    int id, bcap, lanes, groups, waves_bazin, waves_decline;
    bool kernel;
};
#define LCFE_FIT_TIER_ROW(id, BCAP, LANES, GROUPS, WB, WD, KERNEL) {id, BCAP, LANES, GROUPS, WB, WD, KERNEL},
constexpr FitTierRow kFitTierTable[] = {LCFE_FIT_TIERS(LCFE_FIT_TIER_ROW)};
#undef LCFE_FIT_TIER_ROW
constexpr int kFitTiers = (int)(sizeof(kFitTierTable) / sizeof(kFitTierTable[0]));

constexpr int fit_tier_cap(int t) { return kFitTierTable[t].bcap; }
constexpr int kFitMaxRows = fit_tier_cap(kFitTiers - 1);   // a longer band: the object-level kernels (lcfe.hip)
// the tier whose kernels run tier t's list: t itself, or the next one
constexpr int fit_tier_host(int t) { return kFitTierTable[t].kernel ? t : t + 1; }
// the row of the tier of capacity BCAP (id -1: no tier has this capacity; the fit kernels refuse it)
constexpr FitTierRow fit_tier_row(int bcap) {
    for (int t = 0; t < kFitTiers; ++t)
        if (kFitTierTable[t].bcap == bcap) return kFitTierTable[t];
    return FitTierRow{-1, bcap, 0, 0, 0, 0, false};
}

// the tier of a band of m rows (m <= kFitMaxRows); narrow == 0 queues the bands of the tier without kernels on its host's
// list, as if the tier were not there (LCFE_FIT_NARROW=0).  A chain of comparisons against constants, for the device as
// well as the host.
constexpr int fit_tier_of(int m, int narrow) {
#define LCFE_FIT_TIER_OF(id, BCAP, LANES, GROUPS, WB, WD, KERNEL) (m <= BCAP) ? ((KERNEL || narrow) ? id : id + 1):
    return LCFE_FIT_TIERS(LCFE_FIT_TIER_OF) kFitTiers - 1;
#undef LCFE_FIT_TIER_OF
}

// the narrow tier -- the one without kernels -- and what its host needs to know of it
constexpr int fit_narrow_tier() {
    for (int t = 0; t < kFitTiers; ++t)
        if (!kFitTierTable[t].kernel) return t;
    return -1;
}
constexpr int kFitNarrowTier = fit_narrow_tier();
static_assert(kFitNarrowTier >= 0 && kFitNarrowTier + 1 < kFitTiers, "one tier without kernels, and a tier behind it");
constexpr int kFitNarrowHost = fit_tier_host(kFitNarrowTier);
constexpr int kFitNarrowRows = kFitTierTable[kFitNarrowTier].bcap;
constexpr int kFitNarrowLanes = kFitTierTable[kFitNarrowTier].lanes;
constexpr int kFitNarrowGroups = kFitTierTable[kFitNarrowTier].groups;

#define LCFE_FIT_TIER_CHECK(I, BCAP, LANES, GROUPS, WB, WD, KERNEL)                                                             \
    static_assert(kFitTierTable[I].id == I && (I == 0 || fit_tier_cap(I == 0 ? 0 : I - 1) < BCAP), "tiers in the order of their ids and of their capacities"); \
    static_assert(LANES * GROUPS <= 64, "the lane groups of one wavefront");                                                    \
    static_assert(KERNEL ? (WB >= 1 && WD >= 1) : (I == kFitNarrowTier && kFitTierTable[I + 1].kernel), "every tier but one has kernels, and that one's host is the next"); \
    static_assert(fit_tier_of(BCAP, 1) == I && fit_tier_of(BCAP, 0) == fit_tier_host(I) && (I + 1 == kFitTiers || fit_tier_of(BCAP + 1, 1) == I + 1), "fit_tier_of at the tier's cap");
LCFE_FIT_TIERS(LCFE_FIT_TIER_CHECK)
#undef LCFE_FIT_TIER_CHECK

}  // namespace lcfe
