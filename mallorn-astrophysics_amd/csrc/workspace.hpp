// workspace.hpp -- the device workspace of one call (every slot of its header, every region behind it, sized and placed
// by ONE walk) and the arithmetic of a persistent grid.  Plain C++: lcfe.hip's host side and tests/hostsim/workspace.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "feature_sets.hpp"
#include "fit_tier_table.hpp"
#include "gp_tier_table.hpp"

namespace lcfe {

// ---- index lists: per LDS tier (feature sets) and per Gram-matrix tier (GP), then the lists the kernels fill
constexpr int kNumBins = 7;            // up to six tiers + "longer than the largest tier" (bin 6; the sets use bins 0..4 + 6)
constexpr int kNumLists = 2 * kNumBins + 12 + 6;
constexpr int kStatFallbackList = 2 * kNumBins;   // objects the lean statistics kernel hands to the general one
constexpr int kBazinFallbackList = 2 * kNumBins + 1;   // objects with a band longer than the largest fit tier
constexpr int kPowerlawFallbackList = 2 * kNumBins + 2;
constexpr int kStatRetryList = 2 * kNumBins + 3;      // light curves of up to 512 rows the lanes kernels do not take (stat_plan_kernel)
constexpr int kStatL16List = 2 * kNumBins + 4;        // light curves of up to 128 rows whose bands fit 16-row lanes (r, i: 32 rows)
constexpr int kStatL32List = 2 * kNumBins + 5;        // ... 32-row lanes (r, i: 64 rows)
constexpr int kStatL32xList = 2 * kNumBins + 6;       // light curves of up to 256 rows whose bands fit 32-row lanes
constexpr int kStatW16List = 2 * kNumBins + 7;        // ... up to 256 rows, 32-row lanes with 16 lanes per light curve (bands of up to 64 rows, r, i: 128)
constexpr int kStatW32List = 2 * kNumBins + 8;        // ... up to 512 rows, the same
constexpr int kBazinLongList = 2 * kNumBins + 9;      // light curves of more than 1024 rows with a band beyond the largest fit tier
constexpr int kPowerlawLongList = 2 * kNumBins + 10;  // ... with more post-peak rows in a band than the largest fit tier
constexpr int kResearchLongList = 2 * kNumBins + 11;  // light curves whose r band spans more days than the Mexican-hat grid in LDS
static_assert(SetTraits<SET_RESEARCH>::overflow_list == kResearchLongList, "the research set's overflow list");
constexpr int kGpSortedList = 2 * kNumBins + 12;      // + tier (0..5): the 2-D GP tier's light curves, longest first (gp_sort_kernel)
// the tier lists by name: group 0 = the LDS tiers of the feature sets (the list's id is its bin), group 1 = the GP tiers
constexpr int tier_list(int group, int bin) { return group * kNumBins + bin; }
constexpr int gp_list(int tier) { return tier_list(1, tier); }
constexpr int gp_sorted_list(int tier) { return kGpSortedList + tier; }
constexpr int kGpLongList = gp_list(kNumBins - 1);    // light curves beyond the largest Gram-matrix tier
static_assert(kGpNumTiers + 1 == kNumBins, "one bin per tier of gp_tier_table.hpp + the long light curves (gp_bin_of)");
static_assert(SetTraits<SET_GP2D>::long_above == kGpLastCap && SetTraits<SET_GP1D>::long_above == kGpLastCap, "last GP tier");

// ---- header: [0, 1024) ticket counters (8 per set up to the extension set, then the fit lists'), [1024, 2048) counts (the
// lists' lengths, then the fit lists'), [2048, 2304) ticket counters of the registered sets (8 per set)
constexpr size_t kWsHeader = 2304;
constexpr size_t kWsCounts = 1024;                          // byte offset of counts[]
// (kFitTiers band-length tiers of the fit lists: fit_tier_table.hpp)
constexpr int kFitCountBase = 32;                           // counts[32 + t]: length of fit list t
constexpr int kPlCountA = 40, kPlCountB = 48;               // counts[40 + t], counts[48 + t]
// (the ticket counters of the fit lists sit behind those of the numbered sets and the extension set: 8 per set, 13 sets;
// the registered sets, bits 14 on, have theirs behind the bin counts -- SetTraits::ticket_base)
constexpr int kFitTicketBase = 112;                         // tickets[112 + t]
constexpr int kPlTicketA = kFitTicketBase + kFitTiers, kPlTicketB = kPlTicketA + kFitTiers;     // tickets[...]
constexpr int kRegTicketBase = 256, kRegTicketSets = 4;     // tickets[256] on, behind the counts
static_assert(kFitTicketBase >= (SET_ADVANCED + 1) * 8, "fit tickets behind the sets' tickets");
static_assert(kFitCountBase >= kNumLists && kFitCountBase + kFitTiers <= kPlCountA && kPlCountA + kFitTiers <= kPlCountB && kPlCountB + kFitTiers <= 256,
              "count slots of the fit lists");
static_assert(kPlTicketB + kFitTiers <= 128, "ticket slots of the fit lists");
// a light curve with a band beyond the fit tiers goes to the set's object-level kernel while that kernel's largest LDS tier
// takes it (the set table's), and to the long-object tier beyond
constexpr int kFitObjectRows = kTiers[SetTraits<SET_BAZIN>::max_tier];
static_assert(kTiers[SetTraits<SET_POWERLAW>::max_tier] == kFitObjectRows, "one object-level cap for the Bazin and the decline fits");
static_assert(SetTraits<SET_CESIUM>::ticket_base == kRegTicketBase && NUM_ALL_SETS - SET_CESIUM <= kRegTicketSets,
              "ticket counters of the registered sets");
static_assert((SET_ADVANCED + 1) * 8 <= kFitTicketBase && kPlTicketB + kFitTiers <= 128, "ticket counters of the first 1024 bytes");
static_assert(kRegTicketBase * sizeof(unsigned long long) == 2048 && (kRegTicketBase + kRegTicketSets * 8) * sizeof(unsigned long long) <= kWsHeader,
              "ticket counters of the registered sets fit the header, behind the bin counts");

// ---- per-object entries of the fit workspaces
constexpr int kBandOffsets = 8;        // pboff: band offsets inside the object's slice
constexpr int kBazinFits = 6;          // Bazin: one fit per band
constexpr int kPlBands = 3;            // decline fits: bands g, r, i (peak, sstot, kk: one entry each)
constexpr int kPlFitsA = 21;           // ... seven power laws per band
constexpr int kPlFitsB = 6;            // ... the exponential and the linear model per band

// ---- regions, in workspace order
enum WsRegion {
    WS_HEADER, WS_LISTS,
    WS_GP_TIER, WS_GP_TIER_LAST = WS_GP_TIER + kGpNumTiers - 1,                 // + tier: Gram-matrix slabs of the 2-D GP tier
    WS_BAZIN_ROWS, WS_BAZIN_PBOFF, WS_BAZIN_FITS,                               // pt / pf / pe, pboff, fits
    WS_PL_ROWS, WS_PL_PEAK, WS_PL_PBOFF, WS_PL_KK, WS_PL_FITS_A, WS_PL_FITS_B,  // tp / fp, peak / sstot, pboff, kk, fitsA, fitsB
    WS_GP1D,                                                                    // per-band GP: slabs of the long bands
    WS_LONG,                                                                    // + set: slabs of the set's long-object tier
    WS_NUM_REGIONS = WS_LONG + NUM_ALL_SETS
};

// the sizes that come from the kernels' own structures (lcfe.hip fills them in)
struct WsSizes {
    size_t gp_slab[kGpNumTiers];       // by tier: gp_tier_slab_bytes (no bytes for a tier whose matrix is in LDS)
    size_t gp1d_slab;
    size_t long_slab[NUM_ALL_SETS];    // all slabs of the set's long-object tier (0: bit is no set)
};

// Every region rounded up to 256 bytes; a region the mask does not ask for has no bytes (its offset is where it would be).
// The long-object tier's slabs come last: `short_total` is the workspace without them (lcfe_workspace_bytes), `total`
// the one with them (lcfe_workspace_bytes_for) -- a set has them when its light curves can be longer than its tiers take.
struct WsLayout {
    size_t off[WS_NUM_REGIONS], bytes[WS_NUM_REGIONS];
    size_t short_total, total = 0;
    size_t np, no;                     // rows and light curves the regions are sized for: at least one each

    WsLayout(const WsSizes& z, int mask, int64_t n_obj, int64_t n_points, int64_t max_len, bool with_long) {
        np = (size_t)(n_points > 0 ? n_points : 1);
        no = (size_t)(n_obj > 0 ? n_obj : 1);
        const bool gp2d = mask & (1 << SET_GP2D), bazin = mask & (1 << SET_BAZIN), pl = mask & (1 << SET_POWERLAW);
        take(WS_HEADER, kWsHeader);
        take(WS_LISTS, (size_t)(n_obj > 0 ? n_obj : 0) * kNumLists * sizeof(int));
        for (int k = 0; k < kGpNumTiers; ++k) take(WS_GP_TIER + k, gp2d ? z.gp_slab[k] : 0);
        take(WS_BAZIN_ROWS, bazin ? 3 * sizeof(double) * np : 0);
        take(WS_BAZIN_PBOFF, bazin ? kBandOffsets * sizeof(int) * no : 0);
        take(WS_BAZIN_FITS, bazin ? sizeof(int) * kFitTiers * kBazinFits * no : 0);
        take(WS_PL_ROWS, pl ? 2 * sizeof(double) * np : 0);
        take(WS_PL_PEAK, pl ? 2 * kPlBands * sizeof(double) * no : 0);
        take(WS_PL_PBOFF, pl ? kBandOffsets * sizeof(int) * no : 0);
        take(WS_PL_KK, pl ? kPlBands * sizeof(int) * no : 0);
        take(WS_PL_FITS_A, pl ? sizeof(int) * kFitTiers * kPlFitsA * no : 0);
        take(WS_PL_FITS_B, pl ? sizeof(int) * kFitTiers * kPlFitsB * no : 0);
        take(WS_GP1D, (mask & (1 << SET_GP1D)) ? z.gp1d_slab : 0);
        short_total = total;
        for (int s = 0; s < NUM_ALL_SETS; ++s) {
            // (an overflow list can fill from short light curves)
            const bool needs = for_set(s, [&](auto tag) { using T = SetTraits<tag()>; return max_len > T::long_above || T::overflow_list >= 0; });
            take(WS_LONG + s, (with_long && (mask & (1 << s)) && needs) ? z.long_slab[s] : 0);
        }
    }
    char* at(void* ws, int region) const { return (char*)ws + off[region]; }

private:
    void take(int region, size_t b) {
        off[region] = total;
        bytes[region] = b;
        total += (b + 255) & ~(size_t)255;
    }
};

// ---- tiers: the last tier a launch sequence needs is the first whose cap reaches max_len; its launch also writes the
// NaN rows of the longer light curves (bins >= nan_from)
inline int last_tier(int64_t max_len, int max_tier) {
    int last = 0;
    while (last < max_tier && kTiers[last] < max_len) ++last;
    return last;
}
inline int nan_from_of(int ti, int last) { return (ti == last) ? ti + 1 : kNumBins; }
// (the GP sets bin by the rows of the light curve against the Gram-matrix tiers: gp_last_tier of gp_tier_table.hpp)

// ---- workgroups of a persistent launch: as many as the chip holds at once (the occupancy query may say 0: at least one
// per CU), at most `cap` (0: no cap), and no more than there are tickets of `per_ticket` work items.  0: nothing to launch.
inline int64_t grid_for(int num_cu, int per_cu, int64_t cap, int64_t work_items, int per_ticket) {
    int64_t grid = (int64_t)num_cu * (per_cu < 1 ? 1 : per_cu);
    if (cap > 0 && grid > cap) grid = cap;
    if (grid * per_ticket > work_items) grid = (work_items + per_ticket - 1) / per_ticket;
    return (grid < 1) ? 0 : grid;
}

}  // namespace lcfe
