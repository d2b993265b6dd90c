// workspace.cpp -- stand-alone check of csrc/workspace.hpp: the workspace layout over the grid of
// tests/test_workspace_cpu.py and grid_for against hand-computed cases.  Exit status 0 and "workspace OK" when all hold.
//
// The sizes that come from the kernels' structures (WsSizes) are STAND-INS here: the real ones are sizeof()s of the
// device-side working sets in lcfe.hip, which a host build cannot reach.  The stand-ins are deliberately no multiples of
// 256 bytes, so that the rounding of every region is exercised; the real sizes are pinned by test_workspace_cpu.py.  The
// 2-D GP's slabs, one region per tier of csrc/gp_tier_table.hpp, are checked with the table's own sizes as well.
#include <cstdio>
#include <cstdlib>

#include "../../mallorn-astrophysics_amd/csrc/workspace.hpp"

using namespace lcfe;

static int g_failed = 0;
#define CHECK(cond, ...)                                              \
    do {                                                              \
        if (!(cond)) {                                                \
            if (++g_failed <= 20) { printf("FAILED %s: ", #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                             \
    } while (0)

static size_t up256(size_t b) { return (b + 255) / 256 * 256; }

static WsSizes stand_in_sizes() {
    WsSizes z{{0, 400007, 0, 1000001, 2000003, 3000005}, 500009, {}};
    for (int s = 0; s < NUM_ALL_SETS; ++s) z.long_slab[s] = set_known(s) ? 100000 + 4099 * (size_t)s : 0;
    return z;
}

static void check_layout(const WsSizes& z, int mask, int64_t no, int64_t np, int64_t max_len) {
    const WsLayout T(z, mask, no, np, max_len, true), F(z, mask, no, np, max_len, false);
    // every region at a multiple of 256, in the documented order, back to back after rounding, the last one ends at the total
    size_t at = 0;
    for (int r = 0; r < WS_NUM_REGIONS; ++r) {
        CHECK(T.off[r] % 256 == 0, "mask %d region %d offset %zu", mask, r, T.off[r]);
        CHECK(T.off[r] == at, "mask %d region %d at %zu, previous region ends at %zu", mask, r, T.off[r], at);
        at = T.off[r] + up256(T.bytes[r]);
        if (r == WS_GP1D) CHECK(T.short_total == at, "mask %d short_total %zu, regions %zu", mask, T.short_total, at);
    }
    CHECK(T.total == at, "mask %d total %zu, regions end at %zu", mask, T.total, at);
    CHECK(T.off[WS_HEADER] == 0 && T.bytes[WS_HEADER] == 2304 && T.off[WS_LISTS] == 2304, "header");
    // a set that is not in the mask has no region; one that is has its regions
    const bool gp2d = mask & (1 << SET_GP2D), bazin = mask & (1 << SET_BAZIN), pl = mask & (1 << SET_POWERLAW), gp1d = mask & (1 << SET_GP1D);
    for (int k = 0; k < kGpNumTiers; ++k) CHECK(T.bytes[WS_GP_TIER + k] == (gp2d ? z.gp_slab[k] : 0), "mask %d GP slab of tier %d", mask, k);
    for (int r = WS_BAZIN_ROWS; r <= WS_BAZIN_FITS; ++r) CHECK((T.bytes[r] != 0) == bazin, "mask %d Bazin region %d", mask, r);
    for (int r = WS_PL_ROWS; r <= WS_PL_FITS_B; ++r) CHECK((T.bytes[r] != 0) == pl, "mask %d decline-fit region %d", mask, r);
    CHECK(T.bytes[WS_GP1D] == (gp1d ? z.gp1d_slab : 0), "mask %d per-band GP slab", mask);
    for (int s = 0; s < NUM_ALL_SETS; ++s) {
        const bool in_mask = mask & (1 << s);
        const int long_above = (s == SET_GP2D || s == SET_GP1D) ? 767 : (s == SET_BAZIN || s == SET_POWERLAW || s == SET_RESEARCH) ? 1024 : 2048;
        const bool needs = set_known(s) && (max_len > long_above || s == SET_RESEARCH);
        CHECK(T.bytes[WS_LONG + s] == ((in_mask && needs) ? z.long_slab[s] : 0), "mask %d long slabs of set %d at max_len %lld", mask, s,
              (long long)max_len);
        CHECK(F.bytes[WS_LONG + s] == 0, "mask %d set %d: long slabs without with_long", mask, s);
    }
    // the sizes of the fit regions, from the kernels' indexing: np rows and no light curves, at least one each
    const size_t p = (size_t)(np > 0 ? np : 1), o = (size_t)(no > 0 ? no : 1);
    CHECK(T.np == p && T.no == o, "np, no");
    CHECK(T.bytes[WS_LISTS] == (size_t)no * 32 * 4, "lists");
    if (bazin) CHECK(T.bytes[WS_BAZIN_ROWS] == 24 * p && T.bytes[WS_BAZIN_PBOFF] == 32 * o && T.bytes[WS_BAZIN_FITS] == 4 * 5 * 6 * o, "Bazin sizes");
    if (pl)
        CHECK(T.bytes[WS_PL_ROWS] == 16 * p && T.bytes[WS_PL_PEAK] == 48 * o && T.bytes[WS_PL_PBOFF] == 32 * o && T.bytes[WS_PL_KK] == 12 * o &&
                  T.bytes[WS_PL_FITS_A] == 4 * 5 * 21 * o && T.bytes[WS_PL_FITS_B] == 4 * 5 * 6 * o, "decline-fit sizes");
    // without the long-object tier: the same workspace up to where the long slabs start
    for (int r = 0; r < WS_LONG; ++r) CHECK(F.off[r] == T.off[r] && F.bytes[r] == T.bytes[r], "mask %d region %d: with_long moved it", mask, r);
    CHECK(F.total == T.short_total && F.short_total == F.total, "mask %d: short total %zu / %zu", mask, F.total, T.short_total);
}

int main() {
    const WsSizes z = stand_in_sizes();
    const int64_t n_obj[] = {0, 1, 7, 1000}, n_points[] = {0, 1, 63, 120000};
    const int64_t max_len[] = {0, 128, 767, 768, 1024, 1025, 2048, 2049, 16384, 20000};
    int all = 0, n_masks = 0, masks[NUM_ALL_SETS + 2];
    for (int s = 0; s < NUM_ALL_SETS; ++s)
        if (set_known(s)) { masks[n_masks++] = 1 << s; all |= 1 << s; }
    masks[n_masks++] = 0xff;
    masks[n_masks++] = all;
    for (int m = 0; m < n_masks; ++m)
        for (int64_t no : n_obj)
            for (int64_t np : n_points)
                for (int64_t ml : max_len) check_layout(z, masks[m], no, np, ml);
    // the 2-D GP's regions at the table's slab bytes: slabs x matrix x 8 for a tier in global scratch, nothing for one in LDS
    {
        WsSizes zt = z;
        for (int k = 0; k < kGpNumTiers; ++k) {
            const GpTierRow& r = kGpTierTable[k];
            zt.gp_slab[k] = gp_tier_slab_bytes(k);
            CHECK(zt.gp_slab[k] == (r.global_k ? (size_t)r.slabs * gp_store_doubles(r.np) * 8 : 0), "slab bytes of tier %d", k);
        }
        static_assert(WS_GP_TIER_LAST + 1 == WS_BAZIN_ROWS && kGpNumTiers == 6, "one region per tier, in tier order");
        for (int64_t ml : max_len) check_layout(zt, 0xff, 1000, 120000, ml);
        check_layout(zt, 1 << SET_BAZIN, 1000, 120000, 768);
    }
    // one layout by hand: Bazin alone, 7 light curves, 63 rows
    {
        const WsLayout L(z, 1 << SET_BAZIN, 7, 63, 100, true);
        CHECK(L.off[WS_LISTS] == 2304 && L.off[WS_BAZIN_ROWS] == 2304 + 1024 && L.off[WS_BAZIN_PBOFF] == 3328 + 1536 &&
                  L.off[WS_BAZIN_FITS] == 4864 + 256 && L.total == 5120 + 1024, "Bazin by hand: total %zu", L.total);
    }

    // tiers
    CHECK(last_tier(0, 4) == 0 && last_tier(128, 4) == 0 && last_tier(129, 4) == 1 && last_tier(1025, 4) == 4 && last_tier(1025, 3) == 3 &&
              last_tier(20000, 4) == 4, "last_tier");
    CHECK(nan_from_of(2, 2) == 3 && nan_from_of(1, 2) == kNumBins, "nan_from_of");
    CHECK(gp_last_tier(0) == 0 && gp_last_tier(63) == 0 && gp_last_tier(64) == 1 && gp_last_tier(160) == 3 && gp_last_tier(767) == 5 &&
              gp_last_tier(768) == 5, "gp_last_tier");

    // grid_for(num_cu, per_cu, cap, work_items, per_ticket), by hand for a chip of 256 CUs
    struct Case { int num_cu, per_cu; int64_t cap, work; int per_ticket; int64_t grid; const char* what; };
    const Case cases[] = {
        {256, 0, 0, 1000000, 1, 256, "occupancy 0: one workgroup per CU"},
        {256, -3, 0, 1000000, 1, 256, "negative occupancy: the same"},
        {256, 4, 192, 1000000, 1, 192, "cap below the grid"},
        {256, 2, 1024, 1000000, 1, 512, "cap above the grid"},
        {256, 8, 0, 5, 8, 1, "work smaller than one ticket"},
        {256, 8, 0, 0, 8, 0, "no work: no launch"},
        {256, 8, 0, 0, 1, 0, "no work, one item per ticket"},
        {256, 8, 0, 6 * 1000, 8, 750, "Bazin fits of 1000 light curves: 6000 / 8"},
        {256, 8, 0, 6 * 7, 8, 6, "Bazin fits of 7 light curves: ceil(42 / 8)"},
        {256, 8, 0, 21 * 1000, 8, 2048, "two-parameter decline fits of 1000 light curves: 2625 tickets, the chip holds 2048"},
        {256, 8, 0, 21 * 7, 8, 19, "two-parameter decline fits of 7 light curves: ceil(147 / 8)"},
        {256, 8, 0, 125000, 8, 2048, "a streaming set on 125000 light curves"},
        {256, 4, 256, 100, 8, 13, "the statistics fallback grid on 100 light curves: ceil(100 / 8)"},
        {256, 1, 32, 1000, 1, 32, "the object-level fit kernel: 32 workgroups"},
        {256, 2, 0, 300, 1, 300, "a GP tier on 300 light curves"},
    };
    for (const Case& c : cases) {
        const int64_t g = grid_for(c.num_cu, c.per_cu, c.cap, c.work, c.per_ticket);
        CHECK(g == c.grid, "%s: grid_for = %lld, by hand %lld", c.what, (long long)g, (long long)c.grid);
    }
    if (g_failed) { printf("%d checks failed\n", g_failed); return 1; }
    printf("workspace OK\n");
    return 0;
}
