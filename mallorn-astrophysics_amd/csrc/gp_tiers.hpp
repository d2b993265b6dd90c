// gp_tiers.hpp -- the tiers of the 2-D GP (gp.hpp): row capacities, matrix placement, workgroup size, fused sweep,
// occupancy hint and the long-object tier's working set.  Shared by the tier kernels of lcfe.hip and by the device
// probe of the objective (tests/devprobe/gp_probe.hip), so that the probe instantiates gp_eval exactly as a tier does.
#pragma once
#include "gp.hpp"

namespace lcfe {

constexpr int kGpSmallNP = 240;     // matrix in global scratch, two pivot tiles per pass, two 512-thread workgroups per CU
constexpr int kGpMidNP = 512;       // matrix in global scratch, two pivot tiles per pass, one 512-thread workgroup per CU
constexpr int kGpGlobalNP = 768;    // matrix in global scratch, one pivot tile per pass (512..767 rows)

// the 112- and 160-row tiers can keep their matrix in global scratch as well (L2-resident slabs): the LDS then holds
// only the two pivot panels, two to four workgroups share a CU and the sweep takes two pivot tiles per pass.  Measured
// (125,000 objects): serialised, both tiers gain 8-9 %; with the fit kernels running beside the GP (the default
// schedule) the 112-row tier in global scratch gains 1.5 % end to end and the 160-row tier LOSES 5 % -- so only the former.
constexpr bool kGp112Global = true, kGp160Global = false;

template <int NP> struct gp_threads { static constexpr int T = (NP >= 768) ? 1024 : ((NP >= 160) ? 512 : 256); };
// the two global-scratch tiers whose second pivot panel fits LDS sweep two pivot tiles per pass over the matrix
template <int NP, bool GLOBAL_K> struct gp_fuse { static constexpr bool F = GLOBAL_K && NP <= 512; };

// waves per SIMD to leave room for: the 64- and 112-row tiers fit two or more workgroups per CU in LDS,
// so their register budget is halved (the L-BFGS-B driver spills a little, the sweep does not)
template <int NP, bool GLOBAL_K> struct gp_waves { static constexpr int N = (NP <= 64) ? 3 : (GLOBAL_K ? ((NP == 512) ? 2 : 4) : 2); };

// the long-object tier of the 2-D GP: light curves of more than 767 rows, up to kGpLongNP - 1 valid points; Gram matrix AND
// working set (panels, point arrays, optimiser state) in per-workgroup slabs of global scratch
constexpr int kGpLongNP = 2048;
// (no pivot look-ahead: its staging tile is handed over between lanes of one wavefront under wave-level fences, which the
//  tiers rely on for LDS only)
template <int NP> struct gp_working_set { using type = GpLds<NP, gp_threads<NP>::T / 64, false, false, false>; };

}  // namespace lcfe
