// feature_sets.hpp -- dispatch of one object to a feature set, shared by the HIP kernels
// (lcfe.hip) and the host simulation (tests/hostsim).
#pragma once
#include "stage.hpp"
#include "stat.hpp"
#include "fits.hpp"
#include "tde.hpp"
#include "color.hpp"
#include "shape.hpp"
#include "physics.hpp"
#include "gp.hpp"
#include "research.hpp"
#include "ecolor.hpp"
#include "decline.hpp"
#include "advanced.hpp"
#include "cesium.hpp"
#include "fourier.hpp"
#include "gp1d.hpp"

#include <type_traits>

namespace lcfe {

enum { SET_STAT = 0, SET_BAZIN, SET_POWERLAW, SET_TDE, SET_COLOR, SET_SHAPE, SET_PHYSICS, SET_GP2D, SET_GP1D, SET_RESEARCH, SET_ECOLOR,
       SET_DECLINE, NUM_SETS };
// Extension sets: selected by the mask bits from NUM_SETS on, but not part of the public LCFE_NUM_SETS / lcfe_stats /
// LCFE_MASK_ALL / lcfe_implemented_mask() (include/lcfe.h), so that adding one never changes the ABI of the numbered sets.
// Registered sets follow from bit 14 on: they are in no table of include/lcfe.h but the registry (lcfe_set_count /
// lcfe_set_info), so adding one changes no constant an older caller may hold.  Bit 13 stays unassigned for good: callers
// rely on it being unknown.  NUM_ALL_SETS bounds the mask bits; set_known() tells which of them are sets.
enum { SET_ADVANCED = NUM_SETS, SET_UNASSIGNED, SET_CESIUM, SET_FOURIER, NUM_ALL_SETS };
static_assert(SET_UNASSIGNED == 13 && SET_CESIUM == 14 && SET_FOURIER == 15, "bit 13 is a hole; the registered sets start at 14");
// stream of a set when the call forks side streams (lcfe_extract_device): the caller's, or side stream 0, 1 or 2
enum { STREAM_CALLER = -1, STREAM_SIDE0, STREAM_SIDE1, STREAM_SIDE2 };
#ifdef LCFE_GP_PROF
constexpr int GP_NSTATUS = 16;
#else
constexpr int GP_NSTATUS = 4;
#endif

// THE table of the sets: everything the library knows about a set beyond its arithmetic, one row per set.
//   name, columns, status words: what lcfe_set_info reports
//   working memory: the set's structure behind ObjLds<CAP> in SetLds (void: the GP sets have kernels of their own)
//   tier:   largest LDS tier the working memory fits in (160 KiB per workgroup; 3 = 1024 rows, 4 = 2048 rows)
//   chunk:  list entries per ticket (set_kernel): 1 for the heavy-tailed fits, 8 for the cheap streaming sets
//   waves:  minimum waves per SIMD the 128-row tier's register allocation leaves room for: the bounded fits are long
//           dependent fp64 chains, so a second wave per SIMD matters more than keeping every value in a register
//   long:   light curves of more rows than this need the long-object tier
//   stream: see above
//   overflow: index list of the light curves a tier kernel hands to the long-object tier whatever their length (research:
//           an r band of more days than the Mexican-hat grid in LDS; such a set always needs the long slabs), or -1
#define LCFE_SET_TABLE(X)                                                                                                     \
    /* id            name        columns         status        working memory     tier chunk waves long  stream    overflow */ \
    X(SET_STAT,     "stat",     STAT_NCOL,      0,            StatScratch<CAP>,    4,  8,    1,   2048, STREAM_CALLER, -1)    \
    X(SET_BAZIN,    "bazin",    BAZIN_NCOL,     12,           BazinLds<CAP>,       3,  1,    2,   1024, STREAM_SIDE0,  -1)    \
    X(SET_POWERLAW, "powerlaw", POWERLAW_NCOL,  54,           PowerlawLds<CAP>,    3,  1,    2,   1024, STREAM_SIDE1,  -1)    \
    X(SET_TDE,      "tde",      TDE_NCOL,       0,            TdeLds<CAP>,         4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_COLOR,    "color",    COLOR_NCOL,     0,            ColorLds<CAP>,       4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_SHAPE,    "shape",    SHAPE_NCOL,     0,            ShapeLds<CAP>,       4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_PHYSICS,  "physics",  PHYSICS_NCOL,   0,            PhysicsLds<CAP>,     4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_GP2D,     "gp2d",     GP_NCOL,        GP_NSTATUS,   void,               -1,  0,    0,   767,  STREAM_CALLER, -1)    \
    X(SET_GP1D,     "gp1d",     GP1D_NCOL,      GP1D_NSTATUS, void,               -1,  0,    0,   767,  STREAM_SIDE2,  -1)    \
    X(SET_RESEARCH, "research", RESEARCH_NCOL,  1,            ResearchLds<CAP>,    3,  8,    1,   1024, STREAM_SIDE2,  25)    \
    X(SET_ECOLOR,   "ecolor",   ECOLOR_NCOL,    0,            EcolorLds,           4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_DECLINE,  "decline",  DECLINE_NCOL,   0,            DeclineLds,          4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_ADVANCED, "advanced", ADVANCED_NCOL,  1,            AdvancedLds<CAP>,    4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_CESIUM,   "cesium",   CESIUM_NCOL,    0,            CesiumLds<CAP>,      4,  8,    1,   2048, STREAM_SIDE2,  -1)    \
    X(SET_FOURIER,  "fourier",  FOURIER_NCOL,   0,            FourierLds<CAP>,     4,  8,    1,   2048, STREAM_SIDE2,  -1)

// rows of the LDS tiers 0..4 (lcfe.hip bins the light curves by them)
constexpr int kTiers[] = {128, 256, 512, 1024, 2048};

template <int SET> struct SetTraits;
#define LCFE_SET_TRAITS(ID, NAME, NCOLS, NSTATUS, LDS, TIER, CHUNK, WAVES, LONG, STREAM, OVERFLOW)                                  \
    template <> struct SetTraits<ID> {                                                                                        \
        static constexpr const char* name = NAME;                                                                             \
        static constexpr int ncols = NCOLS, nstatus = NSTATUS, max_tier = TIER, chunk = CHUNK, waves128 = WAVES;              \
        static constexpr int long_above = LONG, stream = STREAM, overflow_list = OVERFLOW;                                    \
        /* first of the set's 8 ticket counters: tickets[8 s] up to the extension set; the registered sets (bits 14 on)      \
           continue at tickets[256], behind the bin counts, because tickets[112..128) belong to the fit lists */              \
        static constexpr int ticket_base = (int(ID) <= SET_ADVANCED) ? ID * 8 : 256 + (ID - SET_CESIUM) * 8;                  \
        static constexpr bool per_object = TIER >= 0;   /* runs through SetLds / RunSet */                                    \
        template <int CAP> using Lds = LDS;                                                                                   \
        static_assert(TIER < 0 || LONG == kTiers[TIER < 0 ? 0 : TIER], "the long-object tier starts where the LDS tiers end"); \
    };
LCFE_SET_TABLE(LCFE_SET_TRAITS)
#undef LCFE_SET_TRAITS

// a run-time set id as a compile-time tag: f(SetTag<SET>{}) of the set `set`, `unknown` for an id that is no set
template <int SET> using SetTag = std::integral_constant<int, SET>;
template <class F, class R = std::invoke_result_t<F&, SetTag<0>>>
inline R for_set(int set, F&& f, R unknown = {}) {
    switch (set) {
#define LCFE_SET_CASE(ID, ...) case ID: return f(SetTag<ID>{});
        LCFE_SET_TABLE(LCFE_SET_CASE)
#undef LCFE_SET_CASE
    }
    return unknown;
}
// the same for a run-time LDS tier: f(IntTag<rows of tier ti>{})
template <int N> using IntTag = std::integral_constant<int, N>;
template <class F, class R = std::invoke_result_t<F&, IntTag<128>>>
inline R for_tier(int ti, F&& f) {
    switch (ti) {
        case 0: return f(IntTag<128>{});
        case 1: return f(IntTag<256>{});
        case 2: return f(IntTag<512>{});
        case 3: return f(IntTag<1024>{});
        case 4: return f(IntTag<2048>{});
    }
    return R{};
}
static_assert(kTiers[0] == 128 && kTiers[1] == 256 && kTiers[2] == 512 && kTiers[3] == 1024 && kTiers[4] == 2048, "for_tier");
inline bool set_known(int set) { return for_set(set, [](auto) { return true; }); }
inline int set_ncols(int set) { return for_set(set, [](auto s) { return SetTraits<s()>::ncols; }); }
inline int set_nstatus(int set) { return for_set(set, [](auto s) { return SetTraits<s()>::nstatus; }); }
inline const char* set_name(int set) { return for_set(set, [](auto s) { return SetTraits<s()>::name; }); }

// Wave-shared working memory (LDS on the device) of one object: the staged rows, then the set's own structure.
template <int SET, int CAP>
struct SetLds {
    ObjLds<CAP> obj;
    typename SetTraits<SET>::template Lds<CAP> s;
};

// copy `ncol` wave-shared doubles to the object's output row (coalesced on the device)
template <class W>
LCFE_FN void store_row(const double* src, double* row, int ncol) {
    for (int k = W::lane(); k < ncol; k += W::LANES) row[k] = src[k];
}
template <class W>
LCFE_FN void fill_row_nan(double* row, int ncol) {
    for (int k = W::lane(); k < ncol; k += W::LANES) row[k] = qnan();
}

// policy of one bounded fit inside a wave: on the device the six band fits of a light curve run
// side by side in 8-lane groups; the host simulation runs them one after the other
template <class W> struct FitPolicy { using type = W; };
#if defined(__HIPCC__)
template <> struct FitPolicy<WaveDev> { using type = GroupDev<8>; };
#endif

// One object of a per-object set: stage, compute (the run_object hook next to the set's code), store the row.
template <class W, int SET, int CAP>
struct RunSet {
    static LCFE_FN int run(const ObjIn& in, SetLds<SET, CAP>& ws, double* row, int32_t* st) {
        stage_object<W, CAP>(in, ws.obj);
        const int rc = run_object<W, typename FitPolicy<W>::type>(ws.obj, in, ws.s, st);
        store_row<W>(ws.s.out, row, SetTraits<SET>::ncols);
        W::sync();
        return rc;
    }
};

// The sets with launchers of their own keep their own forms: the fits take the group policy first and the status words
// (written this way the register allocation of their kernels is what it was), the statistics set has its phase probes.
template <class W, int CAP>
struct RunSet<W, SET_BAZIN, CAP> {
    static LCFE_FN int run(const ObjIn& in, SetLds<SET_BAZIN, CAP>& ws, double* row, int32_t* st) {
        stage_object<W, CAP>(in, ws.obj);
        bazin_object<typename FitPolicy<W>::type, W, CAP>(ws.obj, ws.s, st);
        store_row<W>(ws.s.out, row, BAZIN_NCOL);
        W::sync();
        return 0;
    }
};
template <class W, int CAP>
struct RunSet<W, SET_POWERLAW, CAP> {
    static LCFE_FN int run(const ObjIn& in, SetLds<SET_POWERLAW, CAP>& ws, double* row, int32_t* st) {
        stage_object<W, CAP>(in, ws.obj);
        powerlaw_object<typename FitPolicy<W>::type, W, CAP>(ws.obj, ws.s, st);
        store_row<W>(ws.s.out, row, POWERLAW_NCOL);
        W::sync();
        return 0;
    }
};
template <class W, int CAP>
struct RunSet<W, SET_STAT, CAP> {
    static LCFE_FN int run(const ObjIn& in, SetLds<SET_STAT, CAP>& ws, double* row, int32_t*) {
        LCFE_PT0();
        stage_object<W, CAP>(in, ws.obj);
        LCFE_PT(0);
        stat_object<W, typename FitPolicy<W>::type, CAP>(ws.obj, ws.s);
        LCFE_PT0B();
        store_row<W>(ws.s.out, row, STAT_NCOL);
        W::sync();
        LCFE_PT(3);
        return 0;
    }
};

}  // namespace lcfe
